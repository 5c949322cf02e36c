/*
 * vit_hip.h -- C ABI of the MI355X (gfx950) Viterbi hot path: update() + chainback().
 *
 * This is the drop-in boundary.  The reference (williamyang98/ViterbiDecoderCpp) has no FFI layer: its hot path sits
 * behind a C++ template concept (static update()) plus a state object with public fields.  The C++ host layer in
 * include/viterbi_hip/ keeps that surface and forwards to the entry points below; bindings in any other language bind
 * these symbols directly.  Plain pointers and sizes only: no HIP, torch or C++ types.
 *
 * Reference interface each entry point replaces (paths relative to the reference tree):
 *   vit_hip_create            ViterbiDecoder_Core ctor            include/viterbi/viterbi_decoder_core.h:170-177
 *                             (+ ViterbiBranchTable::data()       include/viterbi/viterbi_branch_table.h:64-66,
 *                                ViterbiDecoder_Config            include/viterbi/viterbi_decoder_config.h:11-18)
 *   vit_hip_update_batch      reset() + Decoder::update<sum_t>()  viterbi_decoder_core.h:202-211, viterbi_decoder_scalar.h:29-55
 *   vit_hip_chainback_batch   chainback()                         viterbi_decoder_core.h:214-236
 *   vit_hip_decode_batch      the call pattern reset->update->chainback of examples/run_simple.cpp:76-80
 *   vit_hip_chainback_batch_ex  the same, naming which of a code's chainback kernels runs (no reference counterpart)
 *   vit_hip_pipeline_*        the same pattern over a stream of batches (the benchmark's loop over frames,
 *                             examples/run_benchmark.cpp:266-282, with its two separately timed phases :272-281) scheduled on
 *                             two or three HIP streams; _set_timing/_get_timing report the two phases per batch
 *   vit_hip_update_host       update() on a host-resident Core (streaming, N = R allowed:
 *                                                                 examples/helpers/puncture_code_helpers.h:51)
 *   vit_hip_chainback_host    chainback() on host-resident decision rows
 *   vit_hip_export_decisions  ViterbiDecisionBits rows            viterbi_decoder_core.h:49-83 (m_decisions[t][w])
 *   vit_hip_depuncture_batch  decode_punctured_symbols()          examples/helpers/puncture_code_helpers.h:17-55 (the
 *                             re-insertion of punctured symbols as the erasure value 0, for a whole batch; the update
 *                             itself then runs through vit_hip_update_batch instead of one update() per R symbols)
 *   vit_hip_reset_batch       reset(starting_state)               viterbi_decoder_core.h:202-211, for a batch of decoders
 *   vit_hip_update_batch_resume  update() called again on a decoder that already holds state: the cursor
 *                             m_current_decoded_bit and the metrics carry over
 *                                                                 viterbi_decoder_scalar.h:29-55 (:37-54 the cursor)
 *   vit_hip_decode_tail_biting_batch  tail-biting frames (no tail, the encoder starts in the state its last K-1 bits leave):
 *                             no reference counterpart -- the reference decodes terminated frames only; this call is written
 *                             in terms of its reset / update / chainback (rule below), with _tail_biting_workspace_bytes
 *   vit_hip_decode_stream     one long unterminated stream as overlapped windows: no reference counterpart either (the reference
 *                             decodes one terminated frame per Core); written in terms of its reset / update / chainback (rule
 *                             below), with vit_hip_stream_workspace_bytes
 *   vit_hip_decode_streams    several such streams in lockstep on one shared window grid, with the launches of one
 *                             vit_hip_decode_stream call (rule below), with vit_hip_streams_workspace_bytes
 *   vit_hip_broadcast_table   "Branch table can be shared between multiple decoders"   README.md:14,
 *                             viterbi_branch_table.h:17-18, one decoder per worker examples/run_benchmark.cpp:193-197:
 *                             here the workers are GPUs and the table travels once over RCCL/xGMI
 *   vit_hip_synth_batch       the BER harness's frame generator   examples/run_snr_ber.cpp:311-359,
 *                             examples/helpers/test_helpers.h:17-64, convolutional_encoder_shift_register.h:42-62
 *   vit_hip_count_bit_errors  get_total_bit_errors()              examples/helpers/test_helpers.h:95-104
 *   vit_hip_encode_batch      ConvolutionalEncoder_ShiftRegister / _Lookup   include/viterbi/convolutional_encoder_shift_register.h:42-62,
 *                             convolutional_encoder_lookup.h, for a batch on the caller's bytes (start state, tail-biting, strides)
 *   vit_hip_channel_errors_batch  no reference counterpart: the re-encoded channel symbol error count (rule below)
 *   vit_hip_sync_build / vit_hip_sync_search  no reference counterpart: node synchronisation -- the streams of a set of alignment
 *                             hypotheses (symbol offset, puncture phase, I/Q rotation) from one received buffer, and their ranking by
 *                             that count in one call (rule below), with vit_hip_sync_search_workspace_bytes
 *   vit_hip_marker_search     no reference counterpart: frame synchronisation -- the distance of a sync marker to the decoded bits,
 *                             summed per phase of the frame period, and the phase and polarity it names (rule below)
 *   vit_hip_frames_extract    no reference counterpart: frame extraction -- the frames of the decoded bits cut at that lock, each on a
 *                             byte boundary, complemented, derandomised, the unfinished frame carried to the next call (rule below),
 *                             with vit_hip_frames_capacity
 *   vit_hip_rs_create / vit_hip_rs_decode_batch  no reference counterpart: the outer Reed-Solomon code of a concatenated link --
 *                             bounded-distance decoding over GF(256) of the interleaved codewords of those frames (rule below)
 *
 * Semantics are those of the reference SCALAR strategy (strict '>' decision, wrapping error_t arithmetic,
 * renormalise only when new_metric[0] >= threshold): SURVEY.md section 8(a').  All results are bit-exact.
 *
 * Conventions
 *   - every function returns VIT_HIP_OK (0) or a negative VIT_HIP_ERR_*; no exception crosses the ABI;
 *     vit_hip_last_error() returns a thread-local description of the last failure.
 *   - pointers named d_* are DEVICE pointers on the handle's device; others are host pointers.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Batch calls only enqueue work: no
 *     allocation, no synchronisation, safe to capture into a hipGraph.
 *   - N = 2^(K-1) states, H = N/2, W = max(N/64, 1) 64-bit decision words per step, S = L + K-1 steps per frame.
 *   - threads: the reference keeps one Core per thread and shares the const branch table (examples/run_benchmark.cpp:193-197,
 *     viterbi_branch_table.h:17-18).  Here a handle plays the table's part for the BATCH calls: they read the handle and
 *     write only caller-owned buffers (workspace, outputs), so several threads / streams may issue them on one handle at
 *     once as long as each call in flight has its own workspace.  The HOST-route calls (vit_hip_update_host,
 *     vit_hip_chainback_host) stage through buffers the handle owns, and vit_hip_set_plan / vit_hip_destroy modify it: one
 *     thread at a time per handle for those (one handle per thread, as one Core per thread in the reference).
 */
#ifndef VIT_HIP_H
#define VIT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIT_HIP_OK 0
#define VIT_HIP_ERR_INVALID_ARG (-1)
#define VIT_HIP_ERR_UNSUPPORTED (-2)
#define VIT_HIP_ERR_RUNTIME (-3)     /* a HIP runtime call failed              */
#define VIT_HIP_ERR_NO_DEVICE (-4)   /* no usable GPU: the product path never falls back to the CPU */
#define VIT_HIP_ERR_WORKSPACE (-5)   /* workspace too small / misaligned       */

/* kernel plans (vit_hip_set_plan): which device implementation serves update()/chainback() */
#define VIT_HIP_PLAN_AUTO 0
#define VIT_HIP_PLAN_LDS 1  /* state metrics staged in LDS, one wavefront per contiguous state slab, ballot decisions */
#define VIT_HIP_PLAN_REG 2  /* state metrics resident in VGPRs, frames in pairs, packed 16-bit ACS (K = 2..9, R <= 6).
                               The stock codes are built in; other polynomials: precompiled at install time
                               (vit_hip_precompile: no compiler on the serving host) or vit_hip_set_plan(h, PLAN_REG) compiles
                               an instantiation with hipcc on first use (10-40 s, cached on disk: VIT_HIP_CACHE_DIR)   */
#define VIT_HIP_PLAN_LDS2 3 /* packed frame pair per workgroup, 16 states per thread, four trellis steps per barrier, u32
                               metrics updated in place in LDS (K = 10..16, R <= 6, any polynomials; K = 10: two frame
                               pairs per wavefront)                                                              */

typedef struct vit_hip_decoder* vit_hip_handle;
typedef void* vit_hip_stream_t;

typedef struct vit_hip_info {
    int32_t K, R, soft_bytes, error_bytes;
    int32_t num_states;      /* N */
    int32_t decision_words;  /* W */
    int32_t device;
    int32_t plan;            /* resolved plan (VIT_HIP_PLAN_LDS / _REG / _LDS2) */
    int32_t soft_decision_high, soft_decision_low; /* recovered from the branch table */
    uint32_t polynomials[16];                      /* recovered G[i] (bit 0 and bit K-1 forced to 1), 0 if not linear */
    int32_t table_is_linear;
    int32_t workspace_tile_frames; /* the decision workspace is an array of independent slabs of this many frames: frame f
                                      lives in slab f / tile, which starts vit_hip_workspace_slab_bytes(h, L) * (f / tile)
                                      bytes into the workspace -- a slab-aligned sub-range of a batch can be chained back or
                                      exported on its own by passing that address */
} vit_hip_info;

const char* vit_hip_last_error(void);
int vit_hip_device_count(void);

/* branch_table: host, [R][H] soft_t exactly as ViterbiBranchTable::data() lays it out (rows contiguous, no padding).
 * config: host, 4 x error_t in the order of ViterbiDecoder_Config (max_error, initial_start_error,
 * initial_non_start_error, renormalisation_threshold).  (soft_bytes, error_bytes) must be (2,2) or (1,1).
 * The table must be two-valued (high/low); it is copied, the caller's table need not outlive the handle. */
int vit_hip_create(int K, int R, int soft_bytes, int error_bytes, const void* branch_table, const void* config,
                   int device, vit_hip_handle* out);
int vit_hip_destroy(vit_hip_handle h);
int vit_hip_get_info(vit_hip_handle h, vit_hip_info* info);
/* PLAN_AUTO never compiles anything: it resolves to a built-in plan, or to PLAN_REG for a code whose kernels were precompiled at
 * install time (vit_hip_precompile below: kernels specialised for its polynomials, else the GENERIC kernels of its (K, R)) -- set
 * VIT_HIP_JIT=1 before vit_hip_create to let it compile.  vit_hip_set_plan(h, PLAN_REG) on a handle that runs the generic kernels looks
 * for specialised ones (package cache, user cache, compiler) and keeps the generic ones when there are none. */
int vit_hip_set_plan(vit_hip_handle h, int plan);
/* Install-time instantiation of the register plan for one polynomial set and symbol width (soft_bytes 1 or 2), for hosts that run
 * WITHOUT a compiler.  In the reference the polynomials are a run-time constructor argument of the branch table
 * (include/viterbi/viterbi_branch_table.h:34-55) and any set runs at the compiled <K,R>'s full speed; here the register plan's
 * kernels are specialised per set, so sets outside the eight stock codes are compiled ahead of use: this call writes the code
 * object into `directory` (NULL: the package cache `<directory of libvit_hip.so>/precompiled`, which vit_hip_create consults for
 * every code it has no built-in kernels for -- such a code then runs PLAN_REG from vit_hip_create on, PLAN_AUTO included).
 * Needs hipcc ($VIT_HIP_HIPCC, else /opt/rocm/bin/hipcc) and the kernel sources beside the library, but NO GPU: a build host
 * without a card can run it (python -m viterbidecodercpp_amd.tools.precompile does, for a list of common sets, from build()).
 * An object that already exists is kept.  path_out (optional) receives the file's path.  K = 2..9, R <= 6.
 * ALL polynomials zero names the GENERIC kernels of (K, R) (K = 3 .. 9 with R = 1 .. 4; not K = 6 at an odd rate): one code object that reads the
 * polynomials from its arguments at run time, as the reference's branch table does -- 0.79 - 0.98 of the specialised kernels' rate.  build()
 * installs them, and vit_hip_create falls back to them (PLAN_AUTO included) for every set of those (K, R) that has neither built-in nor
 * precompiled kernels: no such code drops to the compatibility plan on a host without a compiler.  vit_hip_plan_note says "GENERIC". */
int vit_hip_precompile(int K, int R, const uint32_t* polynomials, int soft_bytes, const char* directory, char* path_out,
                       size_t path_capacity);
/* One line of text about the plan the handle runs and -- where that is PLAN_LDS, the compatibility plan -- whether a faster one
 * exists for this (K, R) and how to get it: no combination the header-level is_valid admits lands on the slow plan silently.
 * Thread-local storage, valid until the thread's next call.  (The reference has no counterpart: its strategies are chosen at
 * compile time, include/viterbi/viterbi_decoder_scalar.h:25.) */
const char* vit_hip_plan_note(vit_hip_handle h);

/* Opaque blob carrying everything vit_hip_create needs (header + table + config): the payload broadcast to the other
 * ranks of a node (RCCL over xGMI via torch.distributed) so that every GPU builds an identical decoder. */
size_t vit_hip_blob_bytes(int K, int R, int soft_bytes, int error_bytes);
int vit_hip_pack_blob(int K, int R, int soft_bytes, int error_bytes, const void* branch_table, const void* config,
                      void* blob, size_t blob_bytes);
int vit_hip_create_from_blob(const void* blob, size_t blob_bytes, int device, vit_hip_handle* out);

/* ---- batched, device-resident (the throughput route) --------------------------------------------------------- */

/* bytes of decision workspace needed for `frames` frames of L info bits (layout is plan-specific and opaque). */
size_t vit_hip_workspace_bytes(vit_hip_handle h, size_t frames, size_t L);
/* bytes between consecutive slabs of vit_hip_info.workspace_tile_frames frames inside a workspace.  Not the same as
 * vit_hip_workspace_bytes(h, tile, L): that is rounded up to 256 bytes, the slab stride of PLAN_LDS (the dense reference
 * layout [F][S][W]) is not.  vit_hip_chainback_batch and vit_hip_export_decisions accept any slab address. */
size_t vit_hip_workspace_slab_bytes(vit_hip_handle h, size_t L);

/* reset(start_state) + update() over n_steps trellis steps (n_steps <= L + K-1) for every frame.
 *   d_symbols       [frames][n_steps][R] soft_t, frame-major, step-major, polynomial-minor
 *   d_workspace     >= vit_hip_workspace_bytes(h, frames, L), 256-byte aligned; receives the decision history
 *   d_final_metrics [frames][N] error_t or NULL  (Core::m_metrics "old" buffer after the last swap)
 *   d_renorm_sum    [frames] uint64 or NULL      (update()'s return value)
 *   d_start_state   [frames] uint32 or NULL (=> 0) */
int vit_hip_update_batch(vit_hip_handle h, const void* d_symbols, size_t frames, size_t n_steps, size_t L,
                         void* d_workspace, size_t workspace_bytes, void* d_final_metrics, uint64_t* d_renorm_sum,
                         const uint32_t* d_start_state, vit_hip_stream_t stream);

/* chainback(bytes_out, L, end_state) for every frame from the workspace a full update (n_steps = L+K-1) filled.
 *   d_bytes_out [frames][ceil(L/8)] ; d_end_state [frames] uint32 or NULL (=> 0) */
int vit_hip_chainback_batch(vit_hip_handle h, const void* d_workspace, size_t frames, size_t L, uint8_t* d_bytes_out,
                            const uint32_t* d_end_state, vit_hip_stream_t stream);
/* the same with the kernel named: VIT_HIP_KERNEL_CHAINBACK (what vit_hip_chainback_batch launches) or
 * VIT_HIP_KERNEL_CHAINBACK_ALT, the other chainback kernel of the K = 7 / K = 9 register-plan codes (K = 7: the LDS-ring kernel,
 * 32 registers -- what a pipeline runs BESIDE update waves; K = 9: the cooperative kernel).  Codes with one chainback kernel
 * ignore the choice.  Results are identical; tests and schedulers use it (there is no environment switch). */
int vit_hip_chainback_batch_ex(vit_hip_handle h, const void* d_workspace, size_t frames, size_t L, uint8_t* d_bytes_out,
                               const uint32_t* d_end_state, vit_hip_stream_t stream, int kernel);

/* update over S = L+K-1 steps from state 0, then chainback: both phases enqueued on `stream`. */
int vit_hip_decode_batch(vit_hip_handle h, const void* d_symbols, size_t frames, size_t L, void* d_workspace,
                         size_t workspace_bytes, uint8_t* d_bytes_out, void* d_final_metrics, uint64_t* d_renorm_sum,
                         const uint32_t* d_end_state, vit_hip_stream_t stream);

/* decision history in the reference's layout: d_decisions [frames][n_steps][W] uint64, bit s%64 of word s/64 of row t
 * = decision for next-state s at step t. */
int vit_hip_export_decisions(vit_hip_handle h, const void* d_workspace, size_t frames, size_t n_steps, size_t L,
                             uint64_t* d_decisions, vit_hip_stream_t stream);

/* Depuncturing front-end for punctured codes (DAB, LTE rate matching ...): builds the [frames][symbols_per_frame] soft_t
 * stream vit_hip_update_batch consumes from the symbols that were actually transmitted.
 *   d_punctured     [frames][punctured_per_frame] soft_t, frame-major
 *   d_source_index  [symbols_per_frame] int32: index into the frame's punctured symbols, or < 0 for a punctured position,
 *                   which reads as the erasure value 0 (examples/run_punctured_decoder.cpp:165).  The same map serves every
 *                   frame; for a puncturing mask it is the exclusive prefix sum of the mask where the mask is set.
 *   d_symbols_out   [frames][symbols_per_frame] soft_t
 * The rule: with j = d_source_index[k], out[f][k] = punctured[f][j] where 0 <= j and (size_t)j < punctured_per_frame, else 0.  An entry
 * at or above punctured_per_frame is out of range and reads as the erasure too (the rule vit_hip_sync_build / vit_hip_sync_search and
 * vit_hip_dab_deinterleave_batch keep for the same map); the map need not be monotonic.  The host cannot see the map, the kernel bounds
 * it: whatever the map holds, nothing outside the buffers is read or written.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the output untouched, for a NULL handle, a NULL d_punctured, d_source_index
 * or d_symbols_out, symbols_per_frame not a multiple of R, more than (2^31 - 1) * 256 groups of 8 output symbols (too large for one
 * launch), d_punctured or d_symbols_out not aligned to soft_t, d_source_index not aligned to 4 bytes, d_symbols_out overlapping
 * d_punctured[0 .. frames * punctured_per_frame) or the map.  frames = 0 or symbols_per_frame = 0 returns VIT_HIP_OK with no work
 * (whatever the buffer pointers are).  One kernel on `stream`, nothing allocated or synchronised: the call can be captured into a hipGraph. */
int vit_hip_depuncture_batch(vit_hip_handle h, const void* d_punctured, size_t punctured_per_frame,
                             const int32_t* d_source_index, size_t symbols_per_frame, size_t frames, void* d_symbols_out,
                             vit_hip_stream_t stream);

/* ---- double-buffered decode pipeline --------------------------------------------------------------------------------- */

/* update() is bound by integer issue, chainback() by memory latency: run back to back they leave each other's resource
 * idle.  A pipeline owns the decision workspaces and HIP streams of a stream of batches and schedules them (this is what
 * bench.py times).  submit() only enqueues and returns; batches complete in submit order; the caller's symbol and output
 * buffers of a batch must stay untouched until a later sync() (or until `done_event`, an optional hipEvent_t passed as
 * void*, has fired).  The schedule is fixed at create time from max_frames (vit_hip_pipeline_get_schedule reports it).  Which
 * kernels may share a SIMD is decided from their kernel DESCRIPTORS (vit_hip_get_kernel_resources: the register allocation the
 * wave launcher uses, not the count the code touches), 512 registers and 160 KiB of LDS per SIMD / CU:
 *   - register plan, more than one and at most two update waves per SIMD (4 x CUs x workspace_tile_frames < max_frames <=
 *     2 x that: 65536 frames at K = 7, 9 on an MI355X) whose chainback kernel fits beside two update waves: two workspaces,
 *     the chainback of batch i on a second, high-priority stream beside the update of batch i+1.
 *       K = 7 (2 x 152 registers): the chainback kernel of this schedule is the LDS-ring one (32 registers, 24 KiB of LDS; the
 *         register-ring kernel, 160 registers, stays the kernel of a chainback that runs alone): 65536 x 8192 back to back
 *         4.15 ms per batch -> 3.30 - 3.45 beside the register-ring kernel -> 3.27 - 3.40;
 *         up to THREE update waves per SIMD (3 x 152 + 32): a 98304-frame batch 5.8 -> 5.0 ms;
 *       K = 9, R = 2 (update capped at 240 registers, LDS-streaming chainback 24 registers with its ring in DYNAMIC LDS -- as
 *         static LDS hipcc padded its allocation to 264 and it ran alone on its SIMD): 65536 x 8192 12.8 -> 12.1 ms;
 *   - register plan, at most ONE update wave per SIMD (max_frames <= 4 x CUs x workspace_tile_frames: the 32768-frame share
 *     of an 8-GPU run): THREE workspaces and TWO update streams, so that two update kernels share the SIMDs (a lone wave
 *     issues a packed instruction every 5.3 cycles, two every 4.5) with the chainbacks beside them on the third stream, at a
 *     higher wave priority than the updates (between two staggered update kernels the chainback would otherwise get the issue
 *     slots both leave over and become the bottleneck; here the fast register-ring kernel serves K = 7 too);
 *       K = 7, R = 3 (LTE: update capped at 240, 2 x 240 + 32), K = 7, R = 4 (DAB: 2 x 224 + 32; eight update waves hold 16 KiB
 *         of LDS each, the chainback ring of these codes is 12 KiB) and K = 9, R = 4 (CDMA 2000: 224 registers with the
 *         sub-chunk branch-metric fetch, 8 KiB of LDS per wave) take the same schedule;
 *   - register plan whose update waves leave no registers (or LDS) for a chainback wave beside two of them (no built-in code any
 *     more; a run-time compiled code whose kernels spill past the caps may): ANY batch of more than one wave per SIMD is fed to
 *     the kernels as SUB-BATCHES of one wave per SIMD through the same three-workspace, two-update-stream schedule (timing
 *     records and vit_hip_pipeline_last_workspace are per sub-batch; an error in the middle of a submit() leaves the sub-batches
 *     already enqueued in flight: sync() or destroy the pipeline before touching the buffers);
 *   - PLAN_LDS2 where the update waves a CU's LDS admits leave the chainback kernel's 24 registers on every SIMD (K = 11, 12,
 *     14, 15: four waves of at most 120; K = 13: three of 144): two workspaces, chainback beside the next update (K = 15,
 *     4096 frames: 51.6 -> 50.2 ms per batch; K = 13, 8192 x 4096: 16.4 -> 16.0);
 *   - larger register-plan batches, K = 16 (4 x 128 registers fill the SIMDs) and PLAN_LDS: a chainback in the update's way
 *     costs more than it hides: one stream, update and chainback back to back. */
typedef struct vit_hip_pipeline* vit_hip_pipeline_t;
typedef struct vit_hip_pipeline_schedule {
    int32_t workspaces;             /* decision workspaces owned (2 or 3 by the rules; vit_hip_pipeline_options: 2 .. 4) */
    int32_t update_streams;         /* update kernels that may be in flight at once (1 or 2 by the rules; options: up to 3) */
    int32_t chainback_overlapped;   /* 1: chainbacks run on their own stream beside the next update; 0: back to back */
    int32_t chainback_wave_priority;/* 1: the chainback kernel runs at a higher wave priority than the update kernels */
    size_t overlap_max_frames;      /* largest batch whose chainback is overlapped */
    size_t two_updates_max_frames;  /* largest max_frames that gets the two-update schedule without sub-batches */
    size_t workspace_bytes_each;
    size_t sub_batch_frames;        /* a submitted batch reaches the kernels in sub-batches of at most this many frames
                                       (= max_frames unless the schedule splits); timing records are per sub-batch */
    int32_t chainback_small_kernel; /* 1: overlapped chainbacks run the small-footprint kernel of the code (K = 7: LDS ring, 32 registers) */
    int32_t reserved;
} vit_hip_pipeline_schedule;
int vit_hip_pipeline_create(vit_hip_handle h, size_t max_frames, size_t L, vit_hip_pipeline_t* out);
/* The supported way to pick a schedule other than the library's (A/B measurements, a host that knows what else shares the GPU):
 * every field left at its "rule" value keeps what vit_hip_pipeline_create would choose; the result is what
 * vit_hip_pipeline_get_schedule_v2 reports.  A request the hardware cannot serve (sub-batches for a batch of one wave per SIMD,
 * three update streams without sub-batches, one update stream for sub-batches -- they are fed from two --, back-to-back chainbacks
 * under two or three update streams -- there every chainback runs on the one chainback stream) is ignored field by field, never an
 * error.  `want` == NULL: the rules.  Every row of this contract runs under tests/test_gpu_pipeline_schedules.py.
 * The library reads NO environment variable for its schedules (a build with -DVIT_HIP_EXPERIMENTS does, for scripts/gpu_ab.sh). */
typedef struct vit_hip_pipeline_options {
    uint32_t struct_size;            /* sizeof(vit_hip_pipeline_options) in the caller's build */
    int32_t chainback_overlap;       /* -1 rule; 0 back to back on the update's stream; 1 overlapped whatever the batch size */
    int32_t update_streams;          /*  0 rule; 1, 2 or 3 update kernels in flight (3 only with sub-batches of one wave per SIMD) */
    int32_t sub_batches;             /* -1 rule; 0 never split; 1 split batches of more than one wave per SIMD */
    int32_t workspaces;              /*  0 rule (update_streams + 1); 2..4 */
    int32_t chainback_small_kernel;  /* -1 rule; 0 the code's stand-alone chainback kernel; 1 its small-footprint kernel (K = 7) */
    int32_t chainback_wave_priority; /* -1 rule; 0 / 1 */
} vit_hip_pipeline_options;
int vit_hip_pipeline_create_ex(vit_hip_handle h, size_t max_frames, size_t L, const vit_hip_pipeline_options* want,
                               vit_hip_pipeline_t* out);
int vit_hip_pipeline_submit(vit_hip_pipeline_t p, const void* d_symbols, size_t frames, uint8_t* d_bytes_out,
                            const uint32_t* d_end_state, void* done_event);
int vit_hip_pipeline_sync(vit_hip_pipeline_t p);
int vit_hip_pipeline_destroy(vit_hip_pipeline_t p);
/* schedule_bytes = sizeof(vit_hip_pipeline_schedule) in the CALLER's build: at most that many bytes are written, so a binary
 * built against an older, shorter struct keeps working when the struct grows. */
int vit_hip_pipeline_get_schedule_v2(vit_hip_pipeline_t p, vit_hip_pipeline_schedule* schedule, size_t schedule_bytes);
/* legacy entry point: writes the struct as it was when the symbol was introduced: up to and including `reserved` (the struct
 * already ended in chainback_small_kernel + reserved then), that is offsetof(reserved) + 4 bytes and nothing behind them */
int vit_hip_pipeline_get_schedule(vit_hip_pipeline_t p, vit_hip_pipeline_schedule* schedule);
/* the decision workspace of the most recently submitted (sub-)batch and the frame range of the submitted batch it holds
 * (vit_hip_export_decisions reads the history from it; first_frame / frames may be NULL): valid after a sync() and until the
 * next submit(); owned by the pipeline. */
int vit_hip_pipeline_last_workspace(vit_hip_pipeline_t p, void** d_workspace, size_t* first_frame, size_t* frames);
/* Per-batch timing with HIP events on the streams the kernels run on (the reference times its two phases separately:
 * examples/run_benchmark.cpp:272-281).  set_timing(p, 1) synchronises, clears the records and starts recording every
 * submitted batch; set_timing(p, 0) stops.  get_timing() returns, for the batches completed by the last sync(), in submit
 * order (one record per SUB-batch: vit_hip_pipeline_schedule.sub_batch_frames): the update kernel's duration, the chainback kernel's duration, and the time at which the batch's chainback finished
 * measured from the start of the first recorded update (all in ms; consecutive differences of complete_ms are the
 * pipeline's per-batch step times).  Arrays may be NULL; at most `capacity` entries are written, *n_batches is the count. */
int vit_hip_pipeline_set_timing(vit_hip_pipeline_t p, int enable);
int vit_hip_pipeline_get_timing(vit_hip_pipeline_t p, size_t capacity, float* update_ms, float* chainback_ms, float* complete_ms,
                                size_t* n_batches);

/* Order the NEXT submitted batch behind work of the caller's own stream: its update kernel will not start before `event` (a
 * hipEvent_t passed as void*, recorded by the caller on the stream that produces d_symbols / last used d_bytes_out) has fired.
 * The pipeline runs on private non-blocking streams, so without this (or a device / stream synchronisation) a submit() right
 * after an asynchronous producer of the symbols races with it.  The other direction is submit()'s `done_event`: make the
 * consumer's stream wait on it.  No reference counterpart (the reference is synchronous host code). */
int vit_hip_pipeline_wait_event(vit_hip_pipeline_t p, void* event);

/* ---- what the hardware allocates per wave of a kernel (diagnostics; the pipeline's residency rules read the same table) ---- */

/* From the kernel DESCRIPTOR in the code object (compute_pgm_rsrc1/3, group_segment_fixed_size): the numbers the wave launcher
 * uses to decide which waves share a SIMD / CU.  NOT hipFuncGetAttributes().numRegs, which is the count the code uses: hipcc
 * pads the allocation of kernels whose static LDS limits their occupancy.  No reference counterpart. */
typedef struct vit_hip_kernel_resources {
    uint32_t vgpr_alloc;        /* entries of the SIMD's 512-entry unified register file one wave occupies */
    uint32_t accum_offset;      /* of which architectural VGPRs (the rest are accumulation registers) */
    uint32_t lds_static_bytes;  /* per workgroup, fixed at compile time */
    uint32_t lds_dynamic_bytes; /* per workgroup, added at launch (vit_hip_get_kernel_resources only; 0 from vit_hip_list_kernels) */
    uint32_t scratch_bytes;     /* per lane */
} vit_hip_kernel_resources;
#define VIT_HIP_KERNEL_UPDATE 0
#define VIT_HIP_KERNEL_CHAINBACK 1
#define VIT_HIP_KERNEL_CHAINBACK_ALT 2   /* the other chainback kernel of K = 7 / 9 (vit_hip_chainback_batch_ex) */
#define VIT_HIP_KERNEL_RESUME 3
/* the kernel a handle launches for `kernel` (register plan and PLAN_LDS2; VIT_HIP_ERR_UNSUPPORTED for PLAN_LDS) */
int vit_hip_get_kernel_resources(vit_hip_handle h, int kernel, vit_hip_kernel_resources* out);
/* every kernel of the library's embedded gfx950 code objects, by index (needs no GPU): VIT_HIP_ERR_INVALID_ARG past the end.
 * `name` receives the (mangled) kernel name, truncated to name_capacity - 1 characters. */
int vit_hip_list_kernels(size_t index, char* name, size_t name_capacity, vit_hip_kernel_resources* out);

/* ---- batched streaming: a batch of decoders fed in chunks, state resident on the device ------------------------- */

/* reset(start_state) for every frame: d_metrics [frames][N] error_t <- initial_non_start_error, initial_start_error at the
 * start state (d_start_state [frames] uint32 or NULL => 0). */
int vit_hip_reset_batch(vit_hip_handle h, size_t frames, const uint32_t* d_start_state, void* d_metrics,
                        vit_hip_stream_t stream);

/* update() on decoders that already hold state: NO reset.  Every frame's cursor stands at trellis step `first_step`
 * (= m_current_decoded_bit) and its metrics are in d_metrics_inout [frames][N] error_t; the call consumes n_steps more
 * steps (first_step + n_steps <= L + K-1), writes decision rows [first_step, first_step + n_steps) of the workspace and
 * leaves the new metrics in d_metrics_inout.  A sequence of calls over consecutive step ranges is bit-identical to one
 * vit_hip_update_batch over the whole range (decision rows, metrics, and the renormalisation sums added up).
 *   d_symbols            frame f's chunk starts at d_symbols + f * symbol_frame_stride (in soft_t elements) and holds
 *                        [n_steps][R]; symbol_frame_stride = 0 means n_steps * R (chunks packed back to back)
 *   d_renorm_sum         [frames] uint64 or NULL: update()'s return value for THIS call (not accumulated) */
int vit_hip_update_batch_resume(vit_hip_handle h, const void* d_symbols, size_t symbol_frame_stride, size_t frames,
                                size_t first_step, size_t n_steps, size_t L, void* d_workspace, size_t workspace_bytes,
                                void* d_metrics_inout, uint64_t* d_renorm_sum, vit_hip_stream_t stream);

/* ---- batched tail-biting frames ("wrap-around Viterbi with fixed extension", one pass) ------------------------------------
 * A tail-biting codeword of L info bits x[0..L) is L*R symbols with no tail: the encoder starts in the state x[L-K+1..L) leaves,
 * so the path starts and ends in the same, unknown state (LTE PBCH / PDCCH use the K = 7, R = 1/3 stock code this way).  Rule,
 * bit-exact, in terms of the reference's reset / update / chainback:
 *   - extension: S_ext = head + L + tail steps, ext[e] = symbols[(e - head) mod L] (wraps more than once when L < head);
 *   - metrics: every state starts at initial_start_error (reset() with every state a start state);
 *   - update() over all S_ext steps (the plan's own kernels, resumed from those metrics);
 *   - end state: the smallest final metric, compared as unsigned error_t, the lowest state on a tie;
 *   - chainback(ext_bytes, L_ext = S_ext - (K-1), end_state); the output is bits [head, head + L) of ext_bytes, MSB-first,
 *     ceil(L/8) bytes per frame, pad bits 0;
 *   - d_tail_biting_ok[f] = 1 when ext bits [head-K+1, head) equal ext bits [head+L-K+1, head+L): the decoded path enters and
 *     leaves the window in the same state (a valid tail-biting codeword).
 * L >= K, head >= K-1 and tail >= K-1, else VIT_HIP_ERR_INVALID_ARG and nothing is launched.  8*(K-1) for both (48 at K = 7) is
 * the default of the C++ and Python layers.
 *   d_symbols        [frames][L][R] soft_t
 *   d_workspace      >= vit_hip_tail_biting_workspace_bytes(h, frames, L, head, tail) bytes, 256-byte aligned
 *                    (VIT_HIP_ERR_WORKSPACE otherwise); it holds, each part 256-byte aligned: the plan's decision workspace for
 *                    L_ext at offset 0, the extended symbols, the [frames][N] metrics, the end states, the extended chainback bytes
 *   d_bytes_out      [frames][ceil(L/8)]
 *   d_end_state_out  [frames] uint32 or NULL: the selected end states
 *   d_tail_biting_ok [frames] uint8 or NULL
 * A batch call like the others: it only enqueues (five launches on `stream`), several may be in flight on one handle, each with
 * its own workspace.  vit_hip_tail_biting_workspace_bytes returns 0 for arguments the decode call rejects. */
size_t vit_hip_tail_biting_workspace_bytes(vit_hip_handle h, size_t frames, size_t L, size_t head, size_t tail);
int vit_hip_decode_tail_biting_batch(vit_hip_handle h, const void* d_symbols, size_t frames, size_t L, size_t head,
                                     size_t tail, void* d_workspace, size_t workspace_bytes, uint8_t* d_bytes_out,
                                     uint32_t* d_end_state_out, uint8_t* d_tail_biting_ok, vit_hip_stream_t stream);

/* ---- one long unterminated stream, decoded as overlapped windows ("sliding-window Viterbi with fixed extension", one pass) -------
 * A receiver's continuous convolutionally coded stream has no tail between blocks.  One call decodes one SEGMENT of T trellis steps
 * of it as a batch of overlapping windows on the plan's own update / chainback kernels.  Rule, bit-exact, in terms of the
 * reference's reset / update / chainback, with window W, extension head / tail and flags:
 *   - VIT_HIP_STREAM_BEGIN: step 0 is the encoder's start in state 0 and bits are emitted from bit 0.  Without it the first `head`
 *     steps are lead-in only (the previous call emitted them);
 *   - VIT_HIP_STREAM_END: the last K-1 steps are the zero tail, the end state is 0 and bits are emitted up to T-(K-1).  Without it
 *     the last `tail` steps are look-ahead only: the caller presents them again, with `head` steps before them, as the start of the
 *     next segment (the next segment starts at step T - tail - head of this one);
 *   - emitted range [a, b): a = BEGIN ? 0 : head, b = END ? T-(K-1) : T-tail; n_out = b - a bits, MSB-first, ceil(n_out/8) bytes,
 *     pad bits 0;
 *   - windows: n = max(1, floor((b - head) / W)).  Window i runs steps [i W, i W + head + W + tail) for i < n-1; the last window
 *     runs [(n-1) W, T): it absorbs the remainder and is between one and just under two windows long.  When b - head is a multiple
 *     of W and END is clear all n windows have the same length: a caller that sizes its segments T = head + n W + tail gets one
 *     uniform batch (recommended: the longer last window is a launch of one frame);
 *   - bits: window i emits bits [head + i W, head + (i+1) W) of the segment; window 0 under BEGIN also [0, head); the last window up
 *     to b;
 *   - start metrics: window 0 under BEGIN starts from reset(0); every other window with every state at initial_start_error (the
 *     tail-biting start);
 *   - end state: the last window under END ends in state 0; every other window in the state of smallest final metric, compared as
 *     unsigned error_t, the lowest state on a tie;
 *   - decode: each window runs update() over its steps, then chainback() over steps - (K-1) bits from its end state; its share of
 *     the output is the bit range above, relative to its first step.
 * Arguments: head, tail >= K-1; W >= 8, W >= head, W >= tail (so that every window but the last lies inside the segment under END);
 * b > a; T >= head + tail + (BEGIN ? 0 : 1); T < 2^31 - 16 and (127 W + head + W + tail) * R * sizeof(soft_t) < 2^31 - 2^17 (the
 * launchers' 32-bit counters); no other flag bit.  Everything else is VIT_HIP_ERR_INVALID_ARG and nothing is launched.
 * 8*(K-1) for head and tail and W = 1024 are the defaults of the C++ and Python layers.
 *   d_symbols    [T][R] soft_t, contiguous: the windows are read in place at a stride of W steps (no gather, no copy)
 *   d_workspace  >= vit_hip_stream_workspace_bytes(h, T, W, head, tail, flags) bytes, 256-byte aligned (VIT_HIP_ERR_WORKSPACE
 *                otherwise); it holds, each part 256-byte aligned: the decision workspaces of the uniform windows and of the
 *                longer last window, their [n][N] metrics, end states and chainback bytes
 *   d_bytes_out  [ceil(n_out/8)]
 *   n_bits_out   host, may be NULL: receives n_out (known from the arguments alone: written before the work has run)
 * A batch call like the others: it only enqueues on `stream` -- FIVE launches when every window has the same length (start
 * metrics, update, end-state select, chainback, stitch), up to EIGHT otherwise (a second update, select and chainback for the
 * longer last window; no select for a window that ends in state 0) -- with no allocation and no synchronisation, and can be
 * captured into a hipGraph; several may be in flight on one handle, each with its own workspace.  ONE stream per call: a caller
 * with several streams that advance in lockstep hands them all to vit_hip_decode_streams (below) in one call.
 * Punctured streams need nothing new: vit_hip_depuncture_batch with `frames` = the number of puncturing periods turns the received
 * stream into the contiguous [T][R] buffer this call reads.
 * vit_hip_stream_workspace_bytes returns 0 for arguments the decode call rejects. */
#define VIT_HIP_STREAM_BEGIN 1u
#define VIT_HIP_STREAM_END 2u
size_t vit_hip_stream_workspace_bytes(vit_hip_handle h, size_t T, size_t W, size_t head, size_t tail, unsigned flags);
int vit_hip_decode_stream(vit_hip_handle h, const void* d_symbols, size_t T, size_t W, size_t head, size_t tail, unsigned flags,
                          void* d_workspace, size_t workspace_bytes, uint8_t* d_bytes_out, size_t* n_bits_out,
                          vit_hip_stream_t stream);

/* ---- many lockstep streams in one call, on one shared window grid -----------------------------------------------------------
 * A receiver pushes a few milliseconds at a time -- tens to hundreds of windows -- for several streams at once (the sub-channels
 * of a DAB ensemble, the carriers of a multi-carrier downlink, the virtual channels of a CCSDS link).  One call decodes one
 * segment of EVERY stream with the launches of one vit_hip_decode_stream call.
 *   d_symbols    [n_streams][pitch][R] soft_t: stream s occupies steps [s pitch, s pitch + T); what lies between T and pitch is
 *                padding whose content the result does not depend on (it is read).  The last stream needs only T steps: the
 *                buffer holds (n_streams - 1) pitch + T steps.
 *   d_bytes_out  [n_streams][out_pitch_bytes]
 * Rule, bit-exact: row s of d_bytes_out holds exactly the bytes vit_hip_decode_stream returns for stream s's T steps with the same
 * W, head, tail and flags -- ceil(n_out/8) bytes, pad bits 0; the bytes of a row behind them are not written.  *n_bits_out = n_out
 * as there.  The window bookkeeping of each stream (a, b, n, the longer last window, BEGIN, END) is that of
 * vit_hip_decode_stream, unchanged.  All streams share T, W, head, tail and flags: they run in lockstep.  Per-stream lengths or
 * flags are out of scope (a caller with such streams groups them by shape, or calls vit_hip_decode_stream per stream).
 * How: pitch = m W, so the windows of all streams lie on ONE grid of stride W in the caller's buffer, and the plan's resumed update
 * takes them as one batch of frame stride W R exactly as for one stream.  Between the last uniform window of stream s and the
 * first window of stream s+1 lie m - n_u grid windows that straddle the two segments: these BRIDGE windows are decoded like any
 * other (they read only bytes inside the buffer) and their output is dropped; the last stream's are not launched.  Launched grid
 * windows: (n_streams - 1) m + n_u for n_streams n_u useful ones; with T = head + n W + tail the smallest m is n + 1 (n + 2 when
 * head + tail > W): an overhead of 1/n to 2/n.  The longer last windows of all streams are a second batch of n_streams frames at
 * stride pitch.  When a stream is one window of its own length (n_u = 0) that batch is all there is and the grid is not launched.
 * Arguments: everything vit_hip_decode_stream demands, and n_streams >= 1, pitch >= T, pitch % W == 0, out_pitch_bytes >=
 * ceil(n_out/8); (n_streams - 1) m + n_u and n_streams < 2^31 - 16; with a longer last window and n_streams > 1 on the register
 * plan, pitch * R * sizeof(soft_t) * workspace_tile_frames < 2^31 - 2^17 (the launchers' 32-bit counters).  Everything else is
 * VIT_HIP_ERR_INVALID_ARG and nothing is launched.  Workspace as for one stream (VIT_HIP_ERR_WORKSPACE), sized by
 * vit_hip_streams_workspace_bytes, which returns 0 for arguments the decode call rejects.
 * Launches: the counts of ONE stream whatever n_streams is -- FIVE when every window has one length, at most EIGHT otherwise.  The
 * call only enqueues on `stream`, allocates nothing, synchronises nothing and can be captured into a hipGraph; several may be in
 * flight on one handle, each with its own workspace. */
size_t vit_hip_streams_workspace_bytes(vit_hip_handle h, size_t n_streams, size_t pitch, size_t T, size_t W, size_t head, size_t tail,
                                       unsigned flags);
int vit_hip_decode_streams(vit_hip_handle h, const void* d_symbols, size_t n_streams, size_t pitch, size_t T, size_t W, size_t head,
                           size_t tail, unsigned flags, void* d_workspace, size_t workspace_bytes, uint8_t* d_bytes_out,
                           size_t out_pitch_bytes, size_t* n_bits_out, vit_hip_stream_t stream);

/* ---- multi-GPU set-up for C/C++ hosts ----------------------------------------------------------------------------------- */

/* Broadcast the shared branch table + config from rank `root` to every rank of an RCCL communicator (ncclComm_t passed as
 * void*), over xGMI: the one collective of the multi-GPU path (frames shard with no data-path exchange).  On `root`
 * branch_table / config are inputs, on the other ranks they are outputs ([R][H] soft_t and 4 x error_t); every rank passes
 * the same K, R and widths (template parameters in the reference).  Collective and synchronous on `stream`.  librccl.so is
 * dlopen()ed on first use: the library carries no link-time dependency on RCCL.
 * Failure contract: argument errors are detected alike on every rank before the collective.  A rank whose DATA is bad still
 * enters it (a root that cannot pack or upload the table broadcasts a poisoned header; every rank then returns an error).  The
 * 264 KiB device staging buffer is allocated once per device at the process's first call and kept, so a later call cannot run
 * out of memory in front of the collective.  A rank that has no usable device (hipSetDevice fails, or that one-off allocation
 * fails at the first call) returns VIT_HIP_ERR_NO_DEVICE WITHOUT entering: the caller must then abort the communicator
 * (ncclCommAbort) -- the other ranks are waiting in ncclBroadcast. */
int vit_hip_broadcast_table(void* nccl_comm, int root, int rank, int K, int R, int soft_bytes, int error_bytes,
                            void* branch_table, void* config, int device, vit_hip_stream_t stream);

/* ---- synthetic frames and error counting on the device (test / measurement harness) ----------------------------------- */

/* The reference BER harness's generator for a whole batch, in one kernel: random info bytes -> convolutional encoder
 * (MSB-first bits, K-1 zero tail bits) -> +-1 BPSK + N(0, sigma^2) -> round / clamp to [low, high]
 * (sigma^2 = 10^(-(ebn0_db - 10 log10 R + 3)/10), scale (high-low)/2 / sqrt(1 + sigma^2): run_snr_ber.cpp:319-359).
 * Every value is a pure function of (seed, first_frame + f, position) through Philox4x32-10: splitting a batch over calls
 * or ranks does not change it.  noise_free != 0: symbols are exactly high / low (ebn0_db ignored).
 *   d_tx_bytes [frames][L/8] or NULL (L % 8 == 0) ; d_symbols [frames][L+K-1][R] soft_t
 * high / low are the two values of the handle's branch table.  A table that shows only one of them (K = 2 always: its single
 * half-state reads low) takes high = low + soft_decision_max_error / R from the decoder config, for this call, the encoder and
 * the symbol counts alike (vit_hip_get_info reports it).  L = 0 gives the K - 1 tail steps alone.
 * Errors: VIT_HIP_ERR_INVALID_ARG for a NULL handle or d_symbols, L % 8 != 0, int16 symbols at an odd address, a batch too large
 * for one launch; VIT_HIP_ERR_UNSUPPORTED for a handle whose table is not a convolutional code's; nothing is written then.
 * frames = 0 returns VIT_HIP_OK with no work. */
int vit_hip_synth_batch(vit_hip_handle h, size_t frames, size_t L, uint64_t seed, uint64_t first_frame, float ebn0_db,
                        int noise_free, uint8_t* d_tx_bytes, void* d_symbols, vit_hip_stream_t stream);

/* *d_count (uint64, device) += number of differing bits between two device byte arrays. */
int vit_hip_count_bit_errors(vit_hip_handle h, const uint8_t* d_a, const uint8_t* d_b, size_t n_bytes, uint64_t* d_count,
                             vit_hip_stream_t stream);

/* ---- re-encoding decoded bits on the device: batched encoder and channel symbol error count --------------------------------
 * The decode calls return bytes and nothing about the channel.  The standard measure is the re-encoded channel symbol error rate:
 * encode the decoded bits again, compare with the hard decisions of the received symbols, skip erasures (the FIC / MSC BER a DAB
 * receiver shows; what CCSDS / DVB-S node synchronisation minimises over symbol alignment, puncture phase and inversion; what an
 * LTE PDCCH blind decoder ranks its candidates by).  vit_hip_encode_batch is the reference's encoder
 * (include/viterbi/convolutional_encoder_shift_register.h:42-62, convolutional_encoder_lookup.h) for a batch, on the caller's own
 * bytes; vit_hip_channel_errors_batch re-encodes in registers and counts, so neither the symbols nor an encoded copy leave the
 * card or are written.  Rule, with the handle's K, R, polynomials (vit_hip_info.polynomials) and soft_decision_high / low:
 *   - shape: steps = L + (TAIL ? K-1 : 0) trellis steps per frame, R symbols per step.  Without TAIL the frame is an unterminated
 *     piece of a stream.  Info bit t of a frame is bit 7 - t%8 of byte t/8 (MSB-first, as chainback() writes them); the pad bits
 *     of the last byte are not read as data;
 *   - state numbering is the decoder's -- what d_start_state of vit_hip_update_batch and d_end_state of vit_hip_chainback_batch
 *     mean: bit j of a state, 0 <= j < K-1, is the input bit j+1 steps back.  The register at step t is
 *     (state << 1 | bit_t) & (2^K - 1), and symbol i of step t is parity(reg & G[i]): soft_decision_high for 1, _low for 0;
 *   - start state: d_start_state[f], NULL => 0.  Under TAIL_BITING bit j of the start state is info bit L-1-j (the state the
 *     frame's last K-1 bits leave).  d_end_state_out [frames] may be NULL; it receives the state after the last step (0 under TAIL);
 *   - strides are in elements, as in vit_hip_update_batch_resume: frame f's symbols start at f * symbol_frame_stride soft_t
 *     elements (0 => steps*R), its bytes at f * bytes_frame_stride (0 => ceil(L/8)); a non-zero stride is at least that value.
 *     What lies between two frames is neither read nor written;
 *   - layouts: frames = 1 with flags = 0 and a start state is one segment of vit_hip_decode_stream; frames = n_streams with
 *     symbol_frame_stride = pitch*R and bytes_frame_stride = out_pitch_bytes is vit_hip_decode_streams.  The caller passes
 *     d_symbols + a*R, the first emitted step, and carries the last K-1 emitted bits as the next call's start state;
 *   - counts, per frame, uint32: d_compared[f] = symbols r with 2 r != high + low -- a symbol at the midpoint is an erasure (the 0
 *     vit_hip_depuncture_batch inserts, or a noisy symbol that lands there) and is skipped; d_errors[f] = compared symbols whose
 *     hard decision 2 r > high + low differs from the re-encoded bit.  d_errors is required, d_compared may be NULL.  The call
 *     OVERWRITES both (it zeroes them on `stream`, then adds integer partial sums: the result does not depend on order).
 * Errors: VIT_HIP_ERR_UNSUPPORTED when vit_hip_info.table_is_linear is 0.  VIT_HIP_ERR_INVALID_ARG, with nothing launched and the
 * outputs untouched, for a NULL required pointer, L = 0, both flags, unknown flag bits, TAIL_BITING with L < K or a non-NULL
 * d_start_state, a stride that is too small, steps*R >= 2^32 (and int16 symbols at an odd address, or more than 2^32 - 1 frames).
 * frames = 0 returns VIT_HIP_OK with no work.
 * Batch calls like the others: they only enqueue on `stream` (encode: one launch; channel errors: the memsets and one launch),
 * allocate nothing, synchronise nothing, can be captured into a hipGraph, read the handle and write only caller buffers. */
#define VIT_HIP_ENCODE_TAIL        1u  /* K-1 zero bits follow the L info bits: steps = L + K-1 */
#define VIT_HIP_ENCODE_TAIL_BITING 2u  /* start state = the state the frame's last K-1 bits leave; steps = L; d_start_state must be NULL */
int vit_hip_encode_batch(vit_hip_handle h, const uint8_t* d_bytes, size_t bytes_frame_stride, size_t frames, size_t L,
                         unsigned flags, const uint32_t* d_start_state, void* d_symbols_out, size_t symbol_frame_stride,
                         uint32_t* d_end_state_out, vit_hip_stream_t stream);
int vit_hip_channel_errors_batch(vit_hip_handle h, const void* d_symbols, size_t symbol_frame_stride, const uint8_t* d_bytes,
                                 size_t bytes_frame_stride, size_t frames, size_t L, unsigned flags,
                                 const uint32_t* d_start_state, uint32_t* d_errors, uint32_t* d_compared,
                                 vit_hip_stream_t stream);

/* ---- node synchronisation: rank stream alignment hypotheses in one call ------------------------------------------------------
 * A receiver that has just locked its demodulator does not know which received symbol is output 0 of a trellis step, where the
 * puncturing period starts, or which of the BPSK / QPSK rotations the carrier loop settled in.  The standard answer (CCSDS / DVB-S
 * node synchronisation) is to decode under every hypothesis and keep the one with the lowest re-encoded channel symbol error rate.
 * A hypothesis is (offset, flags): `offset` = the number of received symbols in front of the first symbol of a puncturing period
 * (one number for the symbol alignment within a step AND the puncture phase: callers enumerate 0 .. kept_per_period - 1,
 * unpunctured kept_per_period = R); flags swap I and Q and negate either.  The four QPSK rotations are the flag sets
 * {0, 1|2, 2|4, 1|4} up to the caller's I/Q convention, BPSK inversion is 2|4.
 *
 * The stream of a hypothesis, bit-exact.  d_received [n_received] soft_t; d_source_index [period_symbols] int32 with
 * kept_per_period means what it means for vit_hip_depuncture_batch over ONE puncturing period (period_symbols a multiple of R;
 * entries are < 0 or index the period's kept_per_period transmitted symbols); NULL / 0 / 0 is unpunctured (period_symbols =
 * kept_per_period = R, the identity).  Output symbol k = t R + i, 0 <= k < T R:
 *   p = k / period_symbols, s = source_index[k % period_symbols]; s < 0: the output is 0, the erasure vit_hip_depuncture_batch
 *   inserts (an s >= kept_per_period reads as an erasure too); else j = offset + p kept_per_period + s, jj = j ^ 1 under SWAP_PAIRS
 *   else j, v = received[jj], and if the negate flag for the parity of j (an index into the CALLER's buffer: even / odd are the
 *   demodulator's I / Q) is set, v = clamp(high + low - v, soft_t's min, soft_t's max).  The output is v.
 * The largest jj any hypothesis reads must be < n_received, else VIT_HIP_ERR_INVALID_ARG and nothing is launched.  The hypotheses
 * are a HOST array, so the host checks this -- without reading the map, which lives on the device: with a map, a last, partial
 * period (T R not a multiple of period_symbols) counts as if it read the period's last transmitted symbol.
 *
 * vit_hip_sync_build writes d_symbols_out [n_hyp][pitch][R] (pitch in steps, >= T; steps [T, pitch) are NOT written) in ONE launch.
 * n_hyp <= 64: the hypotheses travel by value in the kernel arguments -- no host-to-device copy, nothing the caller must keep
 * alive, and the call captures into a hipGraph.  n_hyp = 1 with pitch = T is how a receiver turns the hypothesis that won into the
 * contiguous [T][R] stream vit_hip_decode_stream reads.  T R < 2^32.
 *
 * vit_hip_sync_search, by composition (T, W, head, tail and the workspace obey the rules of vit_hip_decode_streams unchanged):
 *   1. build the hypothesis streams at pitch = W ceil(T / W) into the workspace;
 *   2. vit_hip_decode_streams with flags = 0 (mid-stream): the emitted bits are steps [head, T - tail), n_out = T - head - tail
 *      (segments of T = head + n W + tail keep it at five launches);
 *   3. the encoder state in front of the first emitted step is unknown: with skip = 8 ceil((K-1)/8) the re-encoding starts at
 *      emitted bit `skip`, bit j of its start state = emitted bit skip - 1 - j, 0 <= j < K-1 (the decoder's state numbering, as in
 *      vit_hip_encode_batch).  n_out > skip is required;
 *   4. vit_hip_channel_errors_batch with frames = n_hyp, no flags, the symbols from step head + skip at stride pitch R, the bytes from
 *      byte skip / 8, L = n_out - skip and those start states: d_errors / d_compared [n_hyp] are its outputs;
 *   5. d_best[0] (may be NULL) = the hypothesis no other beats: a beats b iff compared_a > 0 and (compared_b == 0 or
 *      errors_a compared_b < errors_b compared_a, in 64-bit integers); on a tie the lower index wins.
 * A TRANSPARENT code (every polynomial of odd weight: Voyager, IS-95A) decodes an inverted stream to inverted bits with the same
 * count: 2|4 ties with 0 exactly when the symbols are symmetric about the midpoint, d_best names the lower index, and the inversion
 * is resolved by the frame marker, not here.  For a type whose midpoint (high + low) / 2 is not 0 the inserted erasures (value 0)
 * count as compared symbols, alike in every hypothesis.
 * Errors: VIT_HIP_ERR_UNSUPPORTED when vit_hip_info.table_is_linear is 0 (search only); VIT_HIP_ERR_INVALID_ARG, with nothing
 * launched and the outputs untouched, for n_hyp outside 1 .. 64, unknown flag bits, period_symbols % R != 0, kept_per_period outside
 * 1 .. period_symbols, a read past n_received, n_out <= skip, a NULL buffer, and whatever vit_hip_decode_streams rejects;
 * VIT_HIP_ERR_WORKSPACE for a workspace below vit_hip_sync_search_workspace_bytes (which returns 0 for arguments the call rejects)
 * or not 256-byte aligned.
 * Batch calls like the others: they only enqueue on `stream`, allocate nothing, synchronise nothing, can be captured into a
 * hipGraph; several may be in flight on one handle, each with its own workspace. */
typedef struct vit_hip_sync_hypothesis { uint32_t offset; uint32_t flags; } vit_hip_sync_hypothesis;
#define VIT_HIP_SYNC_SWAP_PAIRS  1u   /* received symbols 2j and 2j+1 change places (I <-> Q) */
#define VIT_HIP_SYNC_NEGATE_EVEN 2u   /* symbols at an even received index are mirrored about (high+low)/2 */
#define VIT_HIP_SYNC_NEGATE_ODD  4u   /* ... at an odd received index */
int vit_hip_sync_build(vit_hip_handle h, const void* d_received, size_t n_received, const int32_t* d_source_index,
                       size_t period_symbols, size_t kept_per_period, const vit_hip_sync_hypothesis* hypotheses, size_t n_hyp,
                       size_t T, size_t pitch, void* d_symbols_out, vit_hip_stream_t stream);
size_t vit_hip_sync_search_workspace_bytes(vit_hip_handle h, size_t n_hyp, size_t T, size_t W, size_t head, size_t tail);
int vit_hip_sync_search(vit_hip_handle h, const void* d_received, size_t n_received, const int32_t* d_source_index,
                        size_t period_symbols, size_t kept_per_period, const vit_hip_sync_hypothesis* hypotheses, size_t n_hyp,
                        size_t T, size_t W, size_t head, size_t tail, void* d_workspace, size_t workspace_bytes, uint32_t* d_errors,
                        uint32_t* d_compared, uint32_t* d_best, vit_hip_stream_t stream);

/* ---- frame synchronisation: the sync marker's phase and polarity -----------------------------------------------------------------
 * The decode calls return a bit stream; a frame starts where the attached sync marker stands (CCSDS: the 32 bits 0x1ACFFC1D every
 * frame length; DVB-S: 0x47 every 1632 bits), and the marker also settles the inversion that node synchronisation leaves open on a
 * transparent code.  vit_hip_marker_search gives, for every bit phase of the frame period, the Hamming distance of the marker to the
 * stream summed over all frames, and from that the phase, the polarity and a lock quality figure.  Rule, bit-exact:
 *   - bits: bit t of a row is bit 7 - t%8 of byte t/8 (MSB-first, as chainback() writes them).  Row r starts at r * bytes_row_stride
 *     (0 => ceil(n_bits/8); a non-zero stride is at least that).  Pad bits and what lies between rows are never interpreted, and no
 *     byte at or behind ceil(n_bits/8) of a row is read;
 *   - marker: marker_bits = m, 1 <= m <= 64.  Marker bit j (the j-th transmitted, 0 <= j < m) is bit m-1-j of `marker`; the bits of
 *     `marker` above m must be 0;
 *   - history: history_bits = hb, 0 <= hb <= 63.  d_history[r] is a uint64 whose low hb bits are the hb stream bits in front of bit 0
 *     of row r, the latest of them bit 0 (NULL only with hb = 0).  It is to the marker what d_start_state is to
 *     vit_hip_channel_errors_batch: a receiver counts the marker positions that straddle two calls;
 *   - positions: p runs over -hb <= p <= n_bits - m (n_bits + hb >= m is required).  d(p) = #{ j : bit[p + j] != marker bit j },
 *     negative indices read from the history;
 *   - phases: period_bits = P >= 1, phase0 < P is the phase of position 0: position p belongs to phase (phase0 + p) mod P (the
 *     mathematical mod: p may be negative).  distance[r][phase] = the sum of d(p) over the positions of that phase, count[r][phase]
 *     their number;
 *   - output: d_distance [rows][P] uint32 is required, d_count [rows][P] uint32 may be NULL.  Without VIT_HIP_MARKER_ACCUMULATE the
 *     call OVERWRITES both (it zeroes them on `stream`, in a kernel, then adds integer partial sums: the result does not depend on
 *     order, as in vit_hip_channel_errors_batch) and m * ceil((n_bits + hb) / P) < 2^32 is required, so that no sum wraps.  With the flag it adds
 *     to what the buffers hold -- the running totals of a receiver, whose overflow the caller answers for;
 *   - lock: d_lock [rows] (may be NULL; under ACCUMULATE it needs d_count) is computed from the totals as they stand after this
 *     call.  Candidate (phase, upright) has errors = distance[phase], compared = m * count[phase]; (phase, inverted) has errors =
 *     compared - distance[phase].  a beats b iff compared_a > 0 and (compared_b == 0 or errors_a compared_b < errors_b compared_a,
 *     in 64-bit integers) -- the rule of d_best of vit_hip_sync_search; on a tie the lower phase wins, and at one phase upright
 *     before inverted.  inverted = 1: the caller complements the decoded bytes.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL required pointer (d_count NULL with
 * d_lock under ACCUMULATE), m outside 1 .. 64 or marker bits above m, hb > 63 or d_history NULL with hb > 0, n_bits + hb < m,
 * n_bits >= 2^32 - 64, P = 0, P >= 2^31, phase0 >= P, a stride that is too small, unknown flag bits, the overflow bound above (and
 * more than 2^31 - 1 rows).  rows = 0 returns VIT_HIP_OK with no work.
 * A batch call like the others: it only enqueues kernels on `stream` (one that zeroes the totals unless they accumulate, the search,
 * the pick when d_lock is given), allocates nothing, synchronises nothing, can be captured into a hipGraph, and reads the handle only
 * for its device.
 * Out of scope: an aperiodic "first hit under a threshold" search; markers longer than 64 bits; masked patterns such as DVB-S's
 * 0x47 x 7, 0xB8 as ONE pattern -- such a caller searches 0x47 at P = 1632, where the right phase has an error rate of about 1/8
 * against about 1/2 elsewhere, or at P = 13056; which packet of eight carries the 0xB8 is settled behind Reed-Solomon, by
 * vit_hip_dvb_derandomize_batch. */
#define VIT_HIP_MARKER_ACCUMULATE 1u  /* add to the totals in d_distance / d_count instead of overwriting them */
typedef struct vit_hip_marker_lock { uint32_t phase, inverted, errors, compared; } vit_hip_marker_lock;
int vit_hip_marker_search(vit_hip_handle h, const uint8_t* d_bytes, size_t bytes_row_stride, size_t rows, size_t n_bits,
                          uint64_t marker, unsigned marker_bits, const uint64_t* d_history, unsigned history_bits,
                          size_t period_bits, size_t phase0, unsigned flags, uint32_t* d_distance, uint32_t* d_count,
                          vit_hip_marker_lock* d_lock, vit_hip_stream_t stream);

/* ---- frame extraction: aligned, derandomised frames cut at the marker lock ---------------------------------------------------------
 * vit_hip_marker_search names the bit phase of the frame period at which the marker stands and the polarity; a frame almost never
 * starts on a byte of the decoded rows.  vit_hip_frames_extract takes the rows of decoded bytes of one call and, per row, a carry --
 * the bits of the frame the previous call left unfinished --, and writes every frame the two complete together, each from bit 0 of a
 * byte on, and the new carry.  Rule, bit-exact, per row r, with P = period_bits:
 *   - bits: bit t of any row, carry or frame is bit 7 - t%8 of byte t/8.  Row r starts at r * bytes_row_stride (0 => ceil(n_bits/8);
 *     a non-zero stride is at least that); no byte at or behind ceil(n_bits/8) of a row is read;
 *   - carry: c = d_carry_bits_in[r]; a value above P-1 reads as 0.  d_carry_in == NULL: every c = 0, and d_carry_bits_in is not
 *     read.  The carry row r starts at r * carry_row_stride (0 => ceil((P-1)/8); a non-zero stride is at least that), in and out
 *     alike; no byte at or behind ceil(c/8) of a carry row is read.  The logical stream S has total = c + n_bits bits: the c carry
 *     bits, then the row's n_bits;
 *   - phase0 < P is the phase of bit 0 of the ROW, the argument vit_hip_marker_search takes;
 *   - lock: read on the device from d_lock[r], the struct vit_hip_marker_search writes: phi = d_lock[r].phase mod P, inv =
 *     d_lock[r].inverted != 0 (errors and compared are not read).  Whatever the memory holds, the kernel stays inside its buffers;
 *   - first frame start: skip = (phi + c - phase0) mod P (the mathematical mod).  A carry that begins on a frame start gives skip = 0;
 *     after a re-lock to another phase skip > 0, and the stale partial frame is dropped with the bits in front of the new start;
 *   - counts: skip >= total: nf = 0, rem = 0; else nf = (total - skip) div P, rem = (total - skip) mod P.  d_n_frames[r] = nf.
 *     nf <= ceil(n_bits / P) = vit_hip_frames_capacity(n_bits, P); max_frames must be at least that;
 *   - frame f < nf: F[j] = S[skip + f P + j] ^ inv, 0 <= j < P;
 *   - marker distance: marker_bits = m (0: off; m <= 64, m <= P, marker bit j is bit m-1-j of `marker` as in vit_hip_marker_search):
 *     d_marker_errors[r * max_frames + f] (uint32, may be NULL) = #{ j < m : F[j] != marker bit j } -- the per-frame figure a
 *     flywheel needs;
 *   - output: drop_bits = d < P, Q = P - d: output bit k = F[d + k] ^ pad bit k, 0 <= k < Q, with d_pad [ceil(Q/8)] device bytes shared
 *     by all rows (NULL: none; the CCSDS pseudo-random sequence, say), packed into ceil(Q/8) bytes at d_frames + (r * max_frames + f) *
 *     frame_stride_bytes (0 => ceil(Q/8); a non-zero stride is at least that); the pad bits of the last byte are 0.  Bytes behind a
 *     frame inside its stride are NOT written, frames f >= nf (and their marker distances) are NOT written;
 *   - new carry: d_carry_out row r receives the raw bits S[skip + nf P, total) -- not complemented, not padded: the lock may change
 *     -- from bit 0 of byte 0 on, the pad bits of the last byte 0; bytes behind ceil(rem/8) are not written.  d_carry_bits_out[r] =
 *     rem.  In and out are distinct buffers that overlap neither each other nor d_bytes (the caller ping-pongs them): one launch reads
 *     the old carry and writes the new one with no ordering between workgroups.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for NULL d_bytes, d_lock, d_frames, d_n_frames,
 * d_carry_out or d_carry_bits_out, d_carry_in without d_carry_bits_in, P < 8 or P >= 2^31, phase0 >= P, d >= P, m > 64, m > P or
 * marker bits above m, n_bits = 0 or n_bits >= 2^32 - 64, a stride that is too small, max_frames below the capacity, more than
 * 2^31 - 1 rows.  rows = 0 returns VIT_HIP_OK with no work.
 * A batch call like the others: it only enqueues ONE kernel on `stream` (no memset), allocates nothing, synchronises nothing, can be
 * captured into a hipGraph, and reads the handle only for its device.
 * Out of scope: a lock threshold or flywheel policy (the caller decides from d_marker_errors whether to trust a frame); frames of
 * varying length; DVB-S's inverted every-eighth sync byte as part of extraction (vit_hip_dvb_derandomize_batch puts it upright, behind
 * vit_hip_deinterleave_batch and vit_hip_rs_decode_batch). */
size_t vit_hip_frames_capacity(size_t n_bits, size_t period_bits);   /* ceil(n_bits / period_bits); 0 for period_bits = 0 */
int vit_hip_frames_extract(vit_hip_handle h, const uint8_t* d_bytes, size_t bytes_row_stride, size_t rows, size_t n_bits,
                           size_t period_bits, size_t phase0, const vit_hip_marker_lock* d_lock, const uint8_t* d_carry_in,
                           const uint32_t* d_carry_bits_in, size_t carry_row_stride, uint64_t marker, unsigned marker_bits,
                           size_t drop_bits, const uint8_t* d_pad, uint8_t* d_frames, size_t frame_stride_bytes, size_t max_frames,
                           uint32_t* d_n_frames, uint32_t* d_marker_errors, uint8_t* d_carry_out, uint32_t* d_carry_bits_out,
                           vit_hip_stream_t stream);

/* ---- Reed-Solomon decoding: the outer code of a concatenated link, on the frames vit_hip_frames_extract wrote ---------------------
 * A code over GF(256), described as libfec describes one:
 *   gfpoly      the field polynomial with its x^8 term, primitive (0x187 CCSDS, 0x11D DVB); alpha = the element 0x02;
 *   fcr, prim   the roots of the generator are alpha^(prim * (fcr + j)), 0 <= j < nroots; gcd(prim, 255) = 1, fcr <= 254;
 *   nroots      2 .. 64 parity symbols; t = nroots div 2;
 *   pad         virtual fill: n = 255 - pad symbols are transmitted, n > nroots;
 *   dual_basis  0 / 1; 1 only with gfpoly 0x187.
 * Rule, bit-exact and independent of the algorithm:
 *   - codeword: bytes c_0 .. c_(n-1), c_0 the coefficient of x^(n-1) (first transmitted: data first, parity last); valid iff the
 *     polynomial vanishes at all nroots roots;
 *   - dual basis (CCSDS 131.0-B): the stored bytes are Berlekamp-representation symbols: conventional x is stored as the byte whose
 *     bit 7-i is Tr(x * beta^i), beta = alpha^117, i = 0 .. 7.  The kernel maps stored to conventional on the way in and back on the
 *     way out; Hamming distances are those of the stored bytes;
 *   - interleave depth I >= 1: a frame is n * I bytes, symbol i of codeword c is frame byte i * I + c;
 *   - decision: if a valid codeword v at Hamming distance e <= t of the received word exists it is unique: the output is v, the
 *     status e.  Otherwise the output is the received word unchanged and the status -1.  The failure detection is complete.
 * vit_hip_rs_create validates the parameters, builds the tables on the host and uploads them once to the handle's device;
 * vit_hip_rs_destroy frees them (NULL is accepted).  These two are the only calls that allocate or copy.
 * vit_hip_rs_decode_batch:
 *   - input: the layout vit_hip_frames_extract writes: frame (r, f) at d_in + (r * max_frames + f) * frame_stride_bytes (0 => n * I; a
 *     non-zero stride is at least that);
 *   - d_n_frames [rows] on the device, or NULL: all max_frames frames of every row.  Frames f >= d_n_frames[r] are neither read nor
 *     written, and neither are their status entries; a count above max_frames reads as max_frames;
 *   - output: d_out == d_in (in place) or a buffer of the same layout that does not overlap it.  Out of place all n * I bytes of a
 *     decoded frame are written; bytes behind them inside the stride are not;
 *   - d_status: int32 [rows * max_frames * I], entry (r * max_frames + f) * I + c.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL handle, code, d_in, d_out or d_status,
 * a code made for another device, I = 0 or I > 2^24 - 1, a stride below n * I, d_out and d_in that overlap without being equal, more than 2^31 - 1
 * blocks (rows * max_frames * ceil(I / 8)); at create for parameters outside the table above.  rows = 0 or max_frames = 0 returns
 * VIT_HIP_OK with no work.
 * A batch call like the others: it only enqueues ONE kernel on `stream` (no memset), allocates nothing, synchronises nothing, can be
 * captured into a hipGraph behind vit_hip_frames_extract, and reads the handle only for its device.
 * Out of scope: erasure decoding; a GPU Reed-Solomon encoder; symbol sizes other than 8 bits.  DVB-S's Forney (12 x 17) convolutional
 * de-interleaver and its inverted every-eighth sync byte are calls of their own on either side of this one (below): the (204,188)
 * code decodes the packets vit_hip_deinterleave_batch wrote. */
typedef struct vit_hip_rs_params { uint32_t gfpoly, fcr, prim, nroots, pad, dual_basis; } vit_hip_rs_params;
typedef struct vit_hip_rs_code_s* vit_hip_rs_code;
int vit_hip_rs_create(vit_hip_handle h, const vit_hip_rs_params* params, vit_hip_rs_code* out);
void vit_hip_rs_destroy(vit_hip_rs_code code);
int vit_hip_rs_decode_batch(vit_hip_handle h, vit_hip_rs_code code, const uint8_t* d_in, uint8_t* d_out, size_t frame_stride_bytes,
                            size_t rows, size_t max_frames, const uint32_t* d_n_frames, size_t interleave, int32_t* d_status,
                            vit_hip_stream_t stream);

/* ---- the DVB-S outer chain: convolutional de-interleaver in front of Reed-Solomon, energy-dispersal removal behind it -------------
 * Behind the inner code a DVB-S stream is convolutionally (Forney) interleaved: the 204 bytes vit_hip_frames_extract cuts at the sync
 * byte are not a codeword until vit_hip_deinterleave_batch has put every byte back, and behind vit_hip_rs_decode_batch the 187
 * payload bytes still carry the energy-dispersal sequence, which restarts every eighth packet (a fixed pad cannot remove it) where
 * the sync byte is inverted: vit_hip_dvb_derandomize_batch.
 *
 * vit_hip_deinterleave_batch: branches = B >= 2, cell = M >= 1 bytes per delay unit, packet_bytes = n, a multiple of B (DVB-S: 12, 17,
 * 204).  Byte i of every packet rides branch i mod B -- the sync byte branch 0 --, D = (B-1) M B is the longest delay in bytes, H =
 * ceil(D / n) the packets of history (DVB-S: 2244 and 11).  (H + 1) n <= 32768 is required: a block stages H packets and its own in
 * LDS.  Rule, bit-exact, per row r:
 *   - input: packet (r, f) at d_in + (r * max_frames + f) * frame_stride_bytes (0 => n; a non-zero stride is at least n), the layout
 *     vit_hip_frames_extract writes.  nf = min(d_n_frames[r], max_frames); d_n_frames == NULL: all max_frames packets;
 *   - history: row r of d_hist_in starts at r * hist_row_stride (0 => H n; a non-zero stride is at least that; in and out alike) and
 *     holds H packets packed, the newest last, of which the last fill = min(d_fill_in[r], H) are real.  d_hist_in == NULL: every
 *     fill = 0, and d_fill_in is not read.  The logical sequence S is the fill real history packets, then the nf input packets; T =
 *     fill + nf; Sb is its byte stream;
 *   - output: nout = max(0, T - H), written to d_n_out[r].  Byte i of output packet k < nout is Sb[(H + k) n + i - (B-1 - i mod B) M B]
 *     (T - nout = H whenever nout > 0: the index is never negative), at d_out + (r * max_frames + k) * out_stride_bytes (0 => n).
 *     Bytes behind n inside a stride and packets k >= nout are NOT written; the output is compacted from packet 0, so
 *     vit_hip_rs_decode_batch(d_out, d_n_out, interleave = 1) takes it as it stands;
 *   - new history: the last min(H, T) packets of S, right-aligned in row r of d_hist_out; d_fill_out[r] = min(H, T).  The bytes of the
 *     row in front of them are not written.  In and out are distinct buffers that overlap neither each other nor the input (the caller
 *     ping-pongs them, as the carry of vit_hip_frames_extract), d_out overlaps neither the input nor either history, and the count
 *     arrays written (d_n_out, d_fill_out) overlap neither each other nor those read.
 * Whatever the count and fill memory holds, the kernel stays inside its buffers.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL handle, d_in, d_out, d_n_out, d_hist_out
 * or d_fill_out, d_hist_in without d_fill_in, B < 2, M < 1, n not a multiple of B, (H + 1) n > 32768, a stride that is too small,
 * buffers that overlap as said above, more than 2^31 - 1 rows, packets per row or blocks.  rows = 0 or max_frames = 0 returns
 * VIT_HIP_OK with no work.
 *
 * vit_hip_dvb_derandomize_batch: the sequence is that of EN 300 421: 1 + x^14 + x^15, registers 1 .. 15 loaded with 100101010000000,
 * the output reg 14 ^ reg 15 fed back into register 1, bits MSB-first into prbs[0 .. 1502] = 03 F6 08 34 30 B8 A3 93 ... CB; it starts
 * behind the inverted sync byte and runs, its output gated, across the seven upright ones.  Rule per row r:
 *   - input: packets in the layout above with packet_bytes >= 188 (0 stride => packet_bytes), of which only the first 188 bytes are
 *     read (204: the parity stays behind); nf as above;
 *   - group phase: d_phase_in[r] = g in 0 .. 7 is the place of packet 0 of this call in its group of eight; any value >= 8 means
 *     unknown, d_phase_in == NULL all unknown.  An unknown phase is voted from this call's sync bytes: cost(g) = sum over f < nf of
 *     popcount(in[f][0] ^ E(g, f)), E = 0xB8 if (g + f) mod 8 = 0, else 0x47; the lowest cost wins, the lower g on a tie; with nf = 0
 *     it stays unknown.  d_phase_out[r] = (g + nf) mod 8, or 0xFFFFFFFF while unknown (a known g with nf = 0 comes back as it went in);
 *   - output packet f < nf, 188 bytes at d_out + (r * max_frames + f) * out_stride_bytes (0 => 188), with q = (g + f) mod 8: byte 0 =
 *     in[0] ^ 0xFF if q = 0, else in[0] (de-inverted, not forced); byte i, 1 <= i <= 187, = in[i] ^ prbs[188 q + i - 1];
 *     d_sync_errors[r * max_frames + f] (uint32, may be NULL) = popcount(in[0] ^ E(g, f)); where d_rs_status[r * max_frames + f] (int32,
 *     may be NULL: the status vit_hip_rs_decode_batch wrote at interleave 1) is negative, bit 7 of output byte 1 -- the MPEG
 *     transport_error_indicator -- is set.  Packets f >= nf (and their sync errors) and bytes behind 188 inside a stride are NOT written;
 *   - d_out == d_in with equal strides is in place (one workgroup per row: an unknown phase reads every sync byte before one is
 *     rewritten; the fast way is out of place); otherwise the two do not overlap.  d_phase_out does not overlap d_phase_in.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL handle, d_in, d_out or d_phase_out,
 * packet_bytes < 188, a stride that is too small, d_out overlapping d_in otherwise than above, overlapping phase arrays, more than
 * 2^31 - 1 rows, packets per row or blocks.  rows = 0 or max_frames = 0 returns VIT_HIP_OK with no work.
 * Batch calls like the others: each only enqueues ONE kernel on `stream` (no memset), allocates nothing, synchronises nothing, can be
 * captured into a hipGraph around vit_hip_rs_decode_batch, and reads the handle only for its device.
 * Out of scope: code rates other than through the existing depuncturing front end; DVB-S2; erasures handed to the outer code. */
int vit_hip_deinterleave_batch(vit_hip_handle h, const uint8_t* d_in, size_t frame_stride_bytes, size_t rows, size_t max_frames,
                               const uint32_t* d_n_frames, size_t branches, size_t cell, size_t packet_bytes, const uint8_t* d_hist_in,
                               const uint32_t* d_fill_in, size_t hist_row_stride, uint8_t* d_out, size_t out_stride_bytes,
                               uint32_t* d_n_out, uint8_t* d_hist_out, uint32_t* d_fill_out, vit_hip_stream_t stream);
int vit_hip_dvb_derandomize_batch(vit_hip_handle h, const uint8_t* d_in, size_t frame_stride_bytes, size_t packet_bytes, size_t rows,
                                  size_t max_frames, const uint32_t* d_n_frames, const uint32_t* d_phase_in, const int32_t* d_rs_status,
                                  uint8_t* d_out, size_t out_stride_bytes, uint32_t* d_phase_out, uint32_t* d_sync_errors,
                                  vit_hip_stream_t stream);

/* ---- the frame check: batched CRC of a bit range of every frame, and its syndrome against the transmitted field --------------------
 * A corrected Reed-Solomon codeword is a valid one, not necessarily the one sent; a tail-biting decode ranks candidates, it does not
 * accept one.  What decides is the frame's CRC: the CCSDS frame error control field, the CRC-16 behind a DAB FIB, the CRC-16 / CRC-24
 * of LTE (XORed with the RNTI on PDCCH, the antenna mask on PBCH), the CRC-32 of MPEG-2 PSI.  vit_hip_crc_batch computes it where the
 * frames already lie.
 * A code is (width, poly, init, xorout): 1 <= width <= 32, poly without its x^width term, all three below 2^width.  Rule, bit-exact
 * and independent of the algorithm, for n data bits, MSB-first, nothing reflected:
 *   reg = init;  per bit b:  top = (reg >> (width-1)) & 1;  reg = (reg << 1) & (2^width - 1);  if (top ^ b) reg ^= poly;
 *   crc = reg ^ xorout.
 * CRC of ASCII "123456789": CCSDS (16, 0x1021, 0xFFFF, 0) 0x29B1; LTE CRC16 (16, 0x1021, 0, 0) 0x31C3; DAB (16, 0x1021, 0xFFFF, 0xFFFF)
 * 0xD64E; LTE CRC24A (24, 0x864CFB, 0, 0) 0xCDE703; CRC24B (24, 0x800063, 0, 0) 0x23EF52; CRC8 (8, 0x9B, 0, 0) 0xEA; MPEG-2 (32,
 * 0x04C11DB7, 0xFFFFFFFF, 0) 0x0376E6E7.
 *   - input: the layout vit_hip_frames_extract, vit_hip_rs_decode_batch and vit_hip_deinterleave_batch share: frame (r, f) at d_frames +
 *     (r * max_frames + f) * frame_stride_bytes.  With rows = 1 that is the [F][ceil(L/8)] bytes of vit_hip_decode_tail_biting_batch,
 *     FIBs at stride 32, or the first 223 I bytes of a 255 I byte Reed-Solomon frame;
 *   - d_n_frames [rows] on the device, or NULL: all max_frames frames of every row.  Frames f >= d_n_frames[r] are neither read nor
 *     written, and neither are their entries; a count above max_frames reads as max_frames;
 *   - data: bits [first_bit, first_bit + n_bits) of the frame, bit t of a frame being bit 7 - t%8 of byte t/8.  n_bits = 0 is legal:
 *     crc = init ^ xorout;
 *   - d_crc[r * max_frames + f] (may be NULL) = the CRC of the data;
 *   - d_syndrome[r * max_frames + f] (may be NULL) = crc ^ field, the field being the `width` bits behind the data, MSB-first: 0 means
 *     the frame checks; on PDCCH it is the RNTI, on PBCH the antenna mask.  At least one of the two outputs is given;
 *   - frame_stride_bytes: 0 => exactly ceil((first_bit + n_bits (+ width with d_syndrome)) / 8); a non-zero stride is at least that.
 *     Of a frame only the bytes that hold data bits, and with d_syndrome field bits, are read.
 * Whatever the count memory holds, the kernel reads no byte outside the frames it owns and writes only entries of frames f < nf.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL handle, crc or d_frames, both outputs
 * NULL, a width outside 1 .. 32, poly, init or xorout at or above 2^width, first_bit + n_bits + 32 at or above 2^32 - 1, a stride that is
 * too small, outputs that overlap each other or the input, more than 2^31 - 1 rows, frames per row or blocks (256 threads; a frame takes
 * 1 .. 64 of them by its length).  rows = 0 or max_frames = 0 returns VIT_HIP_OK with no work.
 * A batch call like the others: it only enqueues ONE kernel on `stream` (no memset), allocates nothing, synchronises nothing, can be
 * captured into a hipGraph behind vit_hip_rs_decode_batch, and reads the handle only for its device.  There is no object to create:
 * the constants of the code are a handful of scalars worked out on the host per call, the lookup tables are built in LDS by every block.
 * Out of scope: reflected CRCs (CRC-32/ISO-HDLC and kin); widths above 32; per-frame lengths or codes in one call; a GPU-side CRC
 * append; a CRC on the DVB transport-packet route. */
typedef struct vit_hip_crc_params { uint32_t width, poly, init, xorout; } vit_hip_crc_params;
int vit_hip_crc_batch(vit_hip_handle h, const vit_hip_crc_params* crc, const uint8_t* d_frames, size_t frame_stride_bytes,
                      size_t rows, size_t max_frames, const uint32_t* d_n_frames, size_t first_bit, size_t n_bits,
                      uint32_t* d_crc, uint32_t* d_syndrome, vit_hip_stream_t stream);

/* ---- LTE rate de-matching: from the demodulator's soft bits to the symbols the tail-biting decode reads --------------------------
 * PBCH and PDCCH send the K = 7, R = 1/3 tail-biting code through the rate matching of 3GPP TS 36.212 5.1.4.2 and a Gold-sequence
 * scrambler: 120 coded PBCH bits go out as 1920 (16 repetitions that must be ADDED), the 129 of a 43-bit PDCCH candidate as 72, 144, 288
 * or 576.  vit_hip_lte_rate_dematch_batch descrambles, adds the repetitions and writes the [frames][D][3] symbols
 * vit_hip_decode_tail_biting_batch takes, 0 (the erasure of vit_hip_depuncture_batch and vit_hip_channel_errors_batch) where nothing
 * was sent.  The rule is integer-exact and independent of the algorithm.
 * Transmit side, for each coded stream d(i)[0 .. D), i = 0, 1, 2 the polynomial index (the last axis of [D][3]): Rsb = ceil(D / 32),
 * Kpi = 32 Rsb, N_D = Kpi - D; y = N_D NULLs followed by d(i), written row by row into Rsb x 32; the columns permuted with the pattern of
 * the convolutional code (table 5.1.4-2), P = <1,17,9,25,5,21,13,29,3,19,11,27,7,23,15,31,0,16,8,24,4,20,12,28,2,18,10,26,6,22,14,30>, and
 * read column by column: v(i)[c Rsb + r] = y[P[c] + 32 r].  The circular buffer is w = v(0) | v(1) | v(2); e[k] is the k-th non-NULL
 * entry met walking w cyclically from 0: e[k] = w_nonnull[k mod 3D].  map[j], j in [0, 3D), is the decoder-order index q = 3 d + i of
 * the j-th non-NULL entry (D = 32: stream 0 of the map reads d = P; D = 33: 2,18,10,26,6,22,14,30,4,20,12,28,8,24,16,0,32,1,17,...).
 * Receive side, for frame f and output position q:
 *   out[f][q] = clamp(round_shift(sum over k < E_f with map[k mod 3D] = q of s(f,k) * received[base_f + k])),
 * summed in int32 (modulo 2^32), round_shift(x) = (x + ((1 << shift) >> 1)) >> shift (arithmetic), clamp to [clamp_lo, clamp_hi]; an
 * output without a contribution is 0 (through the same clamp).
 *   - base_f = d_offset ? d_offset[f] : f * received_frame_stride, in elements; E_f = min(d_count ? d_count[f] : E_max, E_max), cut
 *     further so that base_f + E_f <= n_received, 0 where base_f >= n_received.  Whatever the count and offset memory holds, nothing
 *     outside d_received[0 .. n_received) is read.  Every frame's 3D outputs are always written;
 *   - s(f,k) = -1 where d_scramble is given and its bit g' = (base_f + k) mod scramble_period (scramble_period = 0: g' = base_f + k)
 *     is set, bit t being bit 7 - t%8 of byte t/8; else +1.  The negation is int32: -(-128) is 128.  The mask holds scramble_period
 *     bits (0: n_received).  Frames at stride E with period E share one mask; offsets into one control region with period 0 use the
 *     region's.
 * soft_t is the handle's symbol type; its code rate must be 1/3.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the output untouched, for a NULL handle, d_received or d_symbols_out, a
 * handle with R != 3, D = 0 or D > 8192, E_max = 0 or E_max >= 2^24, n_received >= 2^32, shift > 15, clamp_lo > clamp_hi or either outside
 * soft_t, without d_offset a stride below E_max or (frames - 1) * stride + E_max > n_received, an output that overlaps the input (or
 * d_offset / d_count), frames * 3 D >= 2^32, d_received or d_symbols_out not aligned to soft_t.  frames = 0 returns VIT_HIP_OK with no
 * work.
 * A batch call like the others: it only enqueues ONE kernel on `stream` (no memset), allocates nothing, needs no workspace, synchronises
 * nothing and can be captured into a hipGraph in front of vit_hip_decode_tail_biting_batch.
 * Out of scope: turbo-code rate matching (the other permutation, bit selection with k0, soft-buffer limits); PDCCH REG de-interleaving
 * and the cyclic shift; per-frame D in one call; a GPU rate matcher; UCI / CQI multiplexing on PUSCH; demodulation. */
int vit_hip_lte_rate_dematch_batch(vit_hip_handle h, const void* d_received, size_t n_received, size_t received_frame_stride,
                                   const uint32_t* d_offset, const uint32_t* d_count, size_t frames, size_t D, size_t E_max,
                                   const uint8_t* d_scramble, size_t scramble_period, unsigned shift, int clamp_lo, int clamp_hi,
                                   void* d_symbols_out /* [frames][D][3] soft_t */, vit_hip_stream_t stream);

/* ---- the DAB receive chain: time de-interleaver and depuncturing in front of the decode, energy dispersal behind it ---------------
 * ETSI EN 300 401 sends every soft bit of a Main Service Channel sub-channel 0 .. 15 Common Interleaved Frames (24 ms each) late
 * (clause 12), punctures the K = 7, R = 1/4 mother code with several vectors in sequence (clause 11; the maps are built by the host
 * layer: dab.py) and XORs the x^9 + x^5 + 1 sequence, restarted every logical frame, onto the bits (clause 10).
 *
 * vit_hip_dab_deinterleave_batch: bit-exact and independent of the algorithm; soft_t is the handle's symbol type and values pass through
 * unchanged.  d(j) is the 4-bit reversal of j (0, 8, 4, 12, 2, 10, 6, 14, 1, 9, 5, 13, 3, 11, 7, 15), H = 15.  Per row r:
 *   - input: received frame (r, f) is n_received soft bits at d_in + r * in_row_stride + f * in_frame_stride, in elements of soft_t
 *     (in_frame_stride = 0 => n_received, in_row_stride = 0 => max_frames * frame stride; non-zero strides are at least those: with a
 *     frame stride of 55296 a sub-channel is read in place out of whole CIFs).  nf = min(d_n_frames[r], max_frames); d_n_frames == NULL:
 *     all max_frames frames;
 *   - history, as vit_hip_deinterleave_batch: row r of d_hist_in starts at r * hist_row_stride elements (0 => H * n_received; in and out
 *     alike) and holds H frames of n_received, packed, the newest last, of which the last fill = min(d_fill_in[r], H) are real.
 *     d_hist_in == NULL: every fill = 0 and d_fill_in is not read.  S is the fill real history frames, then the nf input frames; T =
 *     fill + nf;
 *   - output: nout = max(0, T - H), written to d_n_out[r].  The transmitter sent b[r'][i] = a[r' - d(i mod 16)][i], so logical frame k
 *     is a_k[i] = S[T - nout - H + k + d(i mod 16)][i] = S[k + d(i mod 16)][i] (T - nout = H whenever nout > 0): the frame index never
 *     exceeds T - 1.  With p = d_source_index[q], output symbol q < symbols_per_frame of frame k < nout is a_k[p] where 0 <= p <
 *     n_received, else 0, the erasure of vit_hip_depuncture_batch.  d_source_index == NULL is the identity: it requires
 *     symbols_per_frame == n_received and gives the de-interleaver alone.  Output frame (r, k) lies at d_out + (r * max_frames + k) *
 *     symbols_per_frame; frames k >= nout are NOT written.  With symbols_per_frame = 4 (L + 6) that is the [frames][L + 6][4] buffer
 *     vit_hip_decode_batch reads;
 *   - new history: the last min(H, T) frames of S, right-aligned in row r of d_hist_out; d_fill_out[r] = min(H, T).  The frames of the
 *     row in front of them are not written.  In and out are distinct buffers the caller ping-pongs.
 * Whatever the count, fill and map memory holds, nothing outside the buffers is read or written.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL handle, d_in, d_out, d_n_out, d_hist_out
 * or d_fill_out, d_hist_in without d_fill_in, n_received = 0 or symbols_per_frame = 0, 16 * n_received or symbols_per_frame at or above
 * 2^32, a stride that is too small, a NULL map with symbols_per_frame != n_received, d_in, d_out or a history not aligned to soft_t, the
 * map or a count array not aligned to 4 bytes, d_out overlapping the input, a history or the map, d_hist_out overlapping the input,
 * d_hist_in or the map, count arrays written that overlap each other or those read, more than 2^31 - 1 rows, frames per row or blocks,
 * rows * max_frames * symbols_per_frame at or above 2^32.  rows = 0 or max_frames = 0 returns VIT_HIP_OK with no work.
 *
 * vit_hip_dab_descramble_batch: p[n] = p[n-5] ^ p[n-9] with p[-9 .. -1] = 1, period 511: 0000 0111 1011 1110 ..., as bytes MSB-first 07
 * BE 2E 64 12 9D A3 CF.  Bit t < n_bits of every frame f < nf is in ^ p[t mod 511], bit t being bit 7 - t%8 of byte t/8; the bits at or
 * behind n_bits in the last byte are copied unchanged.  Layout, counts and the "not written" rule are those of vit_hip_crc_batch: frame
 * (r, f) at (r * max_frames + f) * stride, 0 => ceil(n_bits / 8) (in and out each); frames f >= nf are neither read nor written, and of a
 * frame only its ceil(n_bits / 8) bytes.  d_out == d_in with equal strides is in place; otherwise the two do not overlap.  Dispersal is
 * its own inverse.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the output untouched, for a NULL handle, d_in or d_out, n_bits + 32 at or
 * above 2^32 - 1, a stride that is too small, d_out overlapping d_in otherwise than above or overlapping d_n_frames, more than 2^31 - 1
 * rows or frames per row, rows * max_frames * (n_bits / 32 + 2) at or above 2^32.  rows = 0, max_frames = 0 or n_bits = 0 returns
 * VIT_HIP_OK with no work.
 * Batch calls like the others: each only enqueues ONE kernel on `stream` (no memset), allocates nothing, needs no object, workspace or pad
 * buffer, synchronises nothing and can be captured into a hipGraph around vit_hip_decode_batch.
 * Out of scope: the unequal-error-protection profile table (a UEP row is whatever map the caller passes); a fast path for one short
 * push; OFDM demodulation and frequency de-interleaving.  (DAB+ superframes: vit_hip_dabplus_sync / vit_hip_dabplus_au_batch below.) */
int vit_hip_dab_deinterleave_batch(vit_hip_handle h, const void* d_in, size_t in_row_stride, size_t in_frame_stride, size_t rows,
                                   size_t max_frames, const uint32_t* d_n_frames, size_t n_received, const int32_t* d_source_index,
                                   size_t symbols_per_frame, const void* d_hist_in, const uint32_t* d_fill_in, size_t hist_row_stride,
                                   void* d_out, uint32_t* d_n_out, void* d_hist_out, uint32_t* d_fill_out, vit_hip_stream_t stream);
int vit_hip_dab_descramble_batch(vit_hip_handle h, const uint8_t* d_in, size_t frame_stride_bytes, size_t rows, size_t max_frames,
                                 const uint32_t* d_n_frames, size_t n_bits, uint8_t* d_out, size_t out_stride_bytes,
                                 vit_hip_stream_t stream);

/* ---- DAB+ audio superframes (ETSI TS 102 563): Fire-code sync in front of frames_extract, the access-unit table behind rs_decode ------
 * The logical frames the DAB chain returns carry, in a DAB+ sub-channel of index s = 1 .. 24 (B = 24 s bytes a frame), audio superframes
 * of five frames: 120 s bytes, the first 110 s of them data, the rest the parity of s RS(120,110) codewords read out by columns (symbol i
 * of codeword c is byte i s + c: vit_hip_rs_decode_batch with the code (0x11D, fcr 0, prim 1, nroots 10, pad 135) at interleave s).
 * Which frame starts a superframe is marked by nothing but a checksum: bytes 0 .. 1 are the Fire code of bytes 2 .. 10.  Bit t of
 * anything is bit 7 - t%8 of byte t/8.
 * Fire code: the 16-bit CRC with generator x^16 + x^14 + x^13 + x^12 + x^11 + x^5 + x^3 + x^2 + x + 1 (0x782F), register 0 at the start,
 * nothing reflected, no final XOR (vit_hip_crc_params {16, 0x782F, 0, 0}), over bytes 2 .. 10.
 *   hit(frame) = crc == byte0 * 256 + byte1, and bytes 0 .. 10 are not all zero (an all-zero header checks trivially).
 *
 * vit_hip_dabplus_sync: bit-exact and independent of the algorithm.
 *   - input: frame (r, f) at d_frames + r * row_stride + f * frame_stride, in bytes (frame_stride = 0 => frame_bytes, row_stride = 0 =>
 *     max_frames * frame stride; non-zero strides are at least those), frame_bytes >= 11.  Only bytes 0 .. 10 of a frame are read; any base
 *     alignment.  nf = min(d_n_frames[r], max_frames); d_n_frames == NULL: all max_frames frames;
 *   - frame0 < 5: frame f is of phase (frame0 + f) mod 5 (a receiver passes the logical frames it has seen so far, mod 5);
 *   - d_hits [rows][5] and d_count [rows][5] uint32, both required: per phase the frames that hit and the frames looked at.  flags = 0
 *     overwrites them (no memset by the caller), VIT_HIP_MARKER_ACCUMULATE adds to them, as in vit_hip_marker_search;
 *   - d_lock [rows] (may be NULL) is computed from the totals as they stand after the call: candidate p has compared = count[p] and errors =
 *     count[p] - hits[p]; a beats b iff compared_a > 0 and (compared_b == 0 or errors_a * compared_b < errors_b * compared_a), the lower
 *     phase on a tie.  Written: phase = p * 8 * frame_bytes (the bit phase vit_hip_frames_extract reads at period_bits = 40 * frame_bytes
 *     with phase0 = frame0 * 8 * frame_bytes), inverted = 0, errors, compared.  With no hit anywhere phase 0 wins with errors == compared:
 *     that is how a caller sees "not locked".
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL handle, d_frames, d_hits or d_count, unknown
 * flag bits, frame_bytes below 11 or 40 * frame_bytes at or above 2^31, frame0 >= 5, a stride that is too small, a count array, total or
 * lock not aligned to 4 bytes, outputs that overlap each other, the frames or d_n_frames, more than 2^31 - 1 rows or frames per row.
 * rows = 0 returns VIT_HIP_OK with no work.  It enqueues kernels only (zero, search, pick) on `stream`, allocates nothing, synchronises
 * nothing and can be captured into a hipGraph in front of vit_hip_frames_extract.
 *
 * vit_hip_dabplus_au_batch: bit-exact and independent of the algorithm.
 *   - input: superframe (r, f) at d_in + (r * max_frames + f) * frame_stride_bytes (0 => 120 s; otherwise >= 110 s), the layout
 *     vit_hip_frames_extract and vit_hip_rs_decode_batch share.  Only the first 110 s bytes are read.  d_n_frames as above;
 *   - d_rs_status: int32 [rows * max_frames * s] as vit_hip_rs_decode_batch writes it at interleave s, or NULL;
 *   - header: bit 6 of byte 2 is dac_rate, bit 5 sbr_flag.  (dac, sbr) = (0,1): n_aus 2, au_start[0] 5; (1,1): 3 and 6; (0,0): 4 and 8;
 *     (1,0): 6 and 11.  au_start[k], 1 <= k < n_aus, are the 12 bits at bit offset 24 + 12 (k-1); au_start[n_aus] = 110 s.  The header is
 *     consistent iff au_start[k+1] >= au_start[k] + 3 for every k < n_aus (one data byte and the CRC); the superframe is valid iff it is a
 *     Fire-code hit and consistent;
 *   - d_info [rows * max_frames] = fire_ok | consistent << 1 | rs_failed << 2 | (valid ? n_aus : 0) << 4 | byte2 << 8; rs_failed is set
 *     where any of the superframe's s statuses is negative, 0 with d_rs_status == NULL;
 *   - d_au [rows * max_frames][6]: every superframe f < nf gets all six entries written.  In a valid one, for k < n_aus: start =
 *     au_start[k], bytes = au_start[k+1] - au_start[k] - 2, syndrome = the CRC (16, 0x1021, 0xFFFF, 0xFFFF) of those bytes XORed with the
 *     two bytes behind them: 0 where the access unit checks.  Every other entry is {0, 0, 0xFFFFFFFF}.  Superframes at or behind the count
 *     are not read, and neither their entries nor their info word are written.
 * Whatever the header, count and status memory holds, nothing outside the 110 s bytes of a superframe it owns is read.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL handle, d_in, d_info or d_au, s outside
 * 1 .. 24, a non-zero stride below 110 s, an array not aligned to 4 bytes, outputs that overlap each other, the superframes, d_rs_status or
 * d_n_frames, more than 2^31 - 1 rows, frames per row or blocks (256 threads; a superframe takes 384).  rows = 0 or max_frames = 0 returns
 * VIT_HIP_OK with no work.  ONE kernel on `stream` (no memset), no workspace, nothing allocated or synchronised: it can be captured into a
 * hipGraph behind vit_hip_rs_decode_batch.
 * Out of scope: AAC decoding, PAD / X-PAD extraction, compacting the access units into a buffer of their own, DMB and enhanced packet
 * mode, a lock with decay or a flywheel policy, s > 24, UEP. */
typedef struct vit_hip_dabplus_au { uint32_t start, bytes, syndrome; } vit_hip_dabplus_au;
int vit_hip_dabplus_sync(vit_hip_handle h, const uint8_t* d_frames, size_t row_stride, size_t frame_stride, size_t frame_bytes, size_t rows,
                         size_t max_frames, const uint32_t* d_n_frames, unsigned frame0, unsigned flags, uint32_t* d_hits,
                         uint32_t* d_count, vit_hip_marker_lock* d_lock, vit_hip_stream_t stream);
int vit_hip_dabplus_au_batch(vit_hip_handle h, const uint8_t* d_in, size_t frame_stride_bytes, size_t rows, size_t max_frames,
                             const uint32_t* d_n_frames, unsigned s, const int32_t* d_rs_status, uint32_t* d_info,
                             vit_hip_dabplus_au* d_au, vit_hip_stream_t stream);

/* ---- the IEEE 802.11a/g OFDM data path: de-interleave, SIGNAL parse, descramble, FCS ------------------------------------------------
 * The OFDM PHY of 802.11a/g (clause 17; 802.11p / j at half and quarter clock) sends the K = 7, R = 1/2 code (g0 = 133, g1 = 171 octal),
 * punctured to 2/3 and 3/4, through a per-OFDM-symbol bit interleaver, behind a 7-bit self-synchronising scrambler, with a CRC-32 FCS.
 * These three calls stand around vit_hip_decode_batch on a handle of K = 7, R = 2 whose polynomials are, in this ABI's convention (bit
 * k of a polynomial taps the input bit of k steps ago), (109, 79): A[n] = x[n]^x[n-2]^x[n-3]^x[n-5]^x[n-6], B[n] =
 * x[n]^x[n-1]^x[n-2]^x[n-3]^x[n-6].  Decoded bit t of a frame is bit 7 - t%8 of byte t/8.
 * A rate index m = 0 .. 7 stands for 6, 9, 12, 18, 24, 36, 48, 54 Mbit/s: N_BPSC = 1, 1, 2, 2, 4, 4, 6, 6; code rate 1/2, 3/4, 1/2, 3/4,
 * 1/2, 3/4, 2/3, 3/4; N_CBPS = 48 N_BPSC; N_DBPS = 24, 36, 48, 72, 96, 144, 192, 216; SIGNAL RATE bits R1 R2 R3 R4 = 1101, 1111, 0101,
 * 0111, 1001, 1011, 0001, 0011; s = max(N_BPSC / 2, 1).
 * Per-frame uint32 arguments (d_rate, d_n_sym, d_n_steps, d_length) are read at element f * stride of their array, the stride in
 * uint32 elements (0 => 1): with stride 5 they point into the vit_hip_wifi_signal structs vit_hip_wifi_signal_batch wrote.
 *
 * vit_hip_wifi_deinterleave_batch: de-interleaves and depunctures in one gather, bit-exact and independent of the algorithm; soft_t is
 * the handle's symbol type and values pass through unchanged.  It writes the [frames][S][2] buffer vit_hip_decode_batch reads with
 * L = S - 6.
 *   - input: frame f is max_sym * N_CBPS(m_f) soft bits at d_in + f * in_frame_stride (elements; 0 => max_sym * 288; a non-zero stride is
 *     at least max_sym * N_CBPS of the largest rate d_rate allows: 288 with d_rate), OFDM symbols consecutive, each in transmit order;
 *   - m_f = d_rate ? d_rate[f] (any value) : rate; n_sym_f = min(d_n_sym ? d_n_sym[f] : max_sym, max_sym); n_steps_f = min(d_n_steps ?
 *     d_n_steps[f] : n_sym_f * N_DBPS, n_sym_f * N_DBPS, S); a frame with m_f > 7 has n_steps_f = 0;
 *   - for step n < S and output o (0 = A, 1 = B): n >= n_steps_f gives 0, the erasure of vit_hip_depuncture_batch.  Otherwise q = 2 n + o
 *     is the index in the mother code stream and c its place in the punctured one: rate 1/2, c = q; rate 2/3, of every four A1 B1 A2 B2 the
 *     fourth is not sent (output 0), c = 3 (q / 4) + q % 4; rate 3/4, of every six A1 B1 A2 B2 A3 B3 the fourth and fifth are not sent,
 *     c = 4 (q / 6) + (0, 1, 2, -, -, 3)[q % 6].  With y = c / N_CBPS, k = c % N_CBPS: i = (N_CBPS / 16) (k % 16) + k / 16, j = s (i / s) +
 *     (i + N_CBPS - 16 i / N_CBPS) % s (integer divisions), out[f][n][o] = in[f][y N_CBPS + j].  N_CBPS = 48: k = 1 gives j = 3; N_CBPS = 192:
 *     k = 1 gives j = 13; k -> j is a permutation at every rate.
 * Every one of the 2 S outputs of every frame is always written; whatever the rate and count memory holds, nothing outside d_in[f *
 * stride .. + max_sym * N_CBPS(m_f)) is read.  The erasures behind n_steps_f are what lets a decode that ends in state 0 at step S be a
 * decode to the best-connected state at the tail: the encoder is in state 0 only behind the six tail bits at step 16 + 8 LENGTH + 6, and
 * the pad bits behind them are scrambled.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the output untouched, for a NULL handle, d_in or d_symbols_out, a handle
 * with R != 2, rate > 7 without d_rate, with frames > 0 max_sym = 0 or S = 0, max_sym * 288 at or above 2^32, S at or above 2^31 - 1, a
 * stride that is too small, d_in not aligned to soft_t, d_symbols_out or a count array not aligned to 4 bytes, an output that overlaps the
 * input or a count array, frames * 2 S symbols filling 2^32 dwords or more.  frames = 0 returns VIT_HIP_OK with no work.
 *
 * vit_hip_wifi_signal_batch: the SIGNAL field is one BPSK rate-1/2 OFDM symbol: de-interleave it with rate = 0, max_sym = 1, S = 24 and
 * decode with L = 18, which gives 3 bytes a frame.  The parser reads them at d_bytes + f * frame_stride_bytes (0 => 3) and writes d_signal
 * [frames]: decoded bits 0 .. 3 are R1 .. R4 (rate_index; 8 for a pattern not in the table), bit 4 is reserved, bits 5 .. 16 LENGTH, LSB
 * first, bit 17 even parity over bits 0 .. 16.  valid = 1 where the pattern is known, the parity holds, the reserved bit is 0 and length
 * >= 1.  n_steps = 16 + 8 length + 6 and n_sym = ceil(n_steps / N_DBPS) where valid, else both 0: the next stage erases the frame.
 * Errors: INVALID_ARG for a NULL handle, d_bytes or d_signal, a non-zero stride below 3, d_signal not aligned to 4 bytes or overlapping
 * d_bytes, more than 2^31 - 1 blocks.  frames = 0: no work.
 *
 * vit_hip_wifi_data_batch: works on the bytes vit_hip_decode_batch wrote for the DATA field, frame f at d_bytes + f * frame_stride_bytes
 * (0 => ceil((S - 6) / 8)), n_bits = S - 6 decoded bits d[t] a frame.
 *   - scrambler: p[t] = d[t] for t < 7 (the first seven SERVICE bits are zero: these are the sequence itself), p[t] = p[t-4] ^ p[t-7]
 *     behind them, period 127; with p[0..6] = 0000111 the sequence goes on 0 1111 0010 ..., in bytes 0E F2.  u[t] = d[t] ^ p[t];
 *   - len_f = min(d_length[f], max_length), cut further so that 16 + 8 len_f <= n_bits.  PSDU octet g < len_f, bit b (LSB = 0), is
 *     u[16 + 8 g + b], written to d_psdu + f * psdu_stride + g (psdu_stride 0 => max_length); octets at or behind len_f are not written;
 *   - d_status[f] = {length_used = len_f; seed = p[0..6] as a number, p[0] highest (0: no scrambler state gives it; the frame is still
 *     written); service = u[0..15], u[0] lowest (0 from a conforming sender); fcs_syndrome = CRC32(psdu[0 .. len-4)) ^ LE32(psdu[len-4 ..
 *     len)), CRC32 the ISO-HDLC one (zlib): 0 where the frame checks, 0xFFFFFFFF where len_f < 4}.  In transmit order that is the
 *     non-reflected code (32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF) of vit_hip_crc_batch over frame bits 16 .. 16 + 8 (len - 4) of u, XORed
 *     with the 32 bits behind them MSB-first, the whole read backwards: fcs_syndrome is the 32-bit reversal of that syndrome.
 * Whatever d_length holds, nothing outside the ceil(n_bits / 8) bytes of a frame is read.
 * Errors: INVALID_ARG for a NULL handle or buffer, S below 22 or at or above 2^31 - 1, max_length at or above 2^28, a stride below
 * ceil((S - 6) / 8), a non-zero psdu_stride below min(max_length, (S - 22) / 8), d_length or d_status not aligned to 4 bytes, outputs
 * that overlap each other, d_bytes or d_length, more than 2^31 - 1 blocks (256 threads; a frame takes 1 .. 64 of them by the longest PSDU
 * the call allows).  frames = 0: no work.
 * Batch calls like the others: each only enqueues ONE kernel on `stream` (no memset), allocates nothing, needs no workspace, synchronises
 * nothing and can be captured into a hipGraph around vit_hip_decode_batch.
 * Out of scope: synchronisation, channel estimation and demapping; 802.11n/ac (other interleavers, LDPC, BCC with several encoders) and
 * 802.11b; bucketing frames by length; a transmitter on the card; A-MPDU delimiters. */
typedef struct vit_hip_wifi_signal { uint32_t rate_index, length, n_sym, n_steps, valid; } vit_hip_wifi_signal;
typedef struct vit_hip_wifi_status { uint32_t length_used, seed, service, fcs_syndrome; } vit_hip_wifi_status;
int vit_hip_wifi_deinterleave_batch(vit_hip_handle h, const void* d_in, size_t in_frame_stride, size_t frames, size_t max_sym,
                                    unsigned rate, const uint32_t* d_rate, const uint32_t* d_n_sym, const uint32_t* d_n_steps,
                                    size_t count_stride, size_t S, void* d_symbols_out /* [frames][S][2] soft_t */,
                                    vit_hip_stream_t stream);
int vit_hip_wifi_signal_batch(vit_hip_handle h, const uint8_t* d_bytes, size_t frame_stride_bytes, size_t frames,
                              vit_hip_wifi_signal* d_signal, vit_hip_stream_t stream);
int vit_hip_wifi_data_batch(vit_hip_handle h, const uint8_t* d_bytes, size_t frame_stride_bytes, size_t frames, size_t S,
                            const uint32_t* d_length, size_t length_stride, size_t max_length, uint8_t* d_psdu, size_t psdu_stride,
                            vit_hip_wifi_status* d_status, vit_hip_stream_t stream);

/* ---- DVB-T: inner de-interleaver and depuncturing in front of the decode ---------------------------------------------------------------
 * DVB-T (ETSI EN 300 744) sends the K = 7, R = 1/2 code X = 171, Y = 133 octal punctured to 2/3, 3/4, 5/6 or 7/8 (clause 4.3.3),
 * demultiplexed into v bit streams that are bit-interleaved in blocks of 126, and symbol-interleaved over the Nmax data carriers of an
 * OFDM symbol by a permutation H whose direction alternates with the symbol's parity (clause 4.3.4).  Behind the decoder it is the DVB-S
 * outer chain: sync byte 0x47 every 1632 bits (vit_hip_marker_search, vit_hip_frames_extract), vit_hip_deinterleave_batch at (12, 17),
 * RS(204,188), vit_hip_dvb_derandomize_batch.  This call is the front, on a handle of K = 7, R = 2 with the stock polynomials (109, 79) =
 * (133, 171) octal in this ABI's convention: Y is output 0 of a trellis step and X output 1 -- THE SWAP: the standard names X first, the
 * stock code has it second, and the call writes (Y, X) so that a real broadcast decodes with the stock kernels.
 *   mode 0, 1, 2 = 2k, 4k, 8k: Mmax = 2048, 4096, 8192; Nmax = 1512, 3024, 6048; Nr = 11, 12, 13.  v = 2, 4, 6 (QPSK, 16-QAM, 64-QAM,
 *   non-hierarchical).  rate 0 .. 4 = 1/2, 2/3, 3/4, 5/6, 7/8: a period of k = 1, 2, 3, 5, 7 steps sends k + 1 bits, in the order X1 Y1 |
 *   X1 Y1 Y2 | X1 Y1 Y2 X3 | X1 Y1 Y2 X3 Y4 X5 | X1 Y1 Y2 Y3 Y4 X5 Y6 X7.  steps = Nmax v k / (k + 1) per OFDM symbol (1512 at 2k / QPSK /
 *   1/2, 31752 at 8k / 64-QAM / 7/8): every symbol holds whole periods and the puncturing phase restarts with it.
 *   - input: row r at d_in + r * in_row_stride (elements of soft_t, the handle's symbol type; 0 => n_sym * Nmax * v), n_sym OFDM symbols
 *     of Nmax cells in carrier order, v soft bits a cell, e = 0 the first mapped bit: in[r][y][carrier][e].  Pilots and TPS carriers are
 *     not in it.  Values pass through unchanged;
 *   - H: R'_0 = R'_1 = 0, R'_2 = 1, R'_i = (R'_{i-1} >> 1) | (newbit << (Nr - 2)) with newbit the XOR of bits (0, 3) at 2k, (0, 2) at 4k,
 *     (0, 1, 4, 6) at 8k of R'_{i-1}; R_i has bit Nr-2, Nr-3, .., 0 of R'_i at positions 0 7 5 1 8 2 6 9 3 4 (2k), 7 10 5 8 1 2 4 9 0 3 6
 *     (4k), 5 11 3 0 10 8 6 9 2 4 1 7 (8k); for i = 0 .. Mmax - 1, h = (i mod 2) 2^(Nr-1) + R_i is the next H(q) where h < Nmax.
 *     H(0..7) = 0 1024 16 1025 128 1056 2 1280 (2k), 0 2048 64 2176 1024 2080 256 2050 (4k), 0 4096 128 4128 2048 4104 1 5120 (8k);
 *     sum(q H(q)) mod 65521 = 52702, 9494, 57713;
 *   - parity of symbol y of row r: (first_r + y) & 1 with first_r = d_parity_in ? d_parity_in[r] : parity.  Interleaver cell q is on
 *     carrier P(q) = H(q) in an even symbol, H^-1(q) in an odd one.  With d_parity_out, d_parity_out[r] = first_r + n_sym: the counter
 *     travels between two arrays like the fill of vit_hip_deinterleave_batch, so a captured graph of two calls replays correctly;
 *   - output: row r at d_symbols_out + r * out_row_stride * 2 elements (out_row_stride in trellis steps; 0 => n_sym * steps), symbol y's
 *     steps at y * steps: the `pitch` layout of vit_hip_decode_streams, or one row for vit_hip_decode_stream.  For step n of a symbol and
 *     output o (0 = Y, 1 = X): with j = n mod k, place = (1/2: X 0, Y 1; 2/3: X1 0, Y1 1, Y2 2; 3/4: .., X3 3; 5/6: .., Y4 4, X5 5; 7/8:
 *     X1 0, Y1 1, Y2 2, Y3 3, Y4 4, X5 5, Y6 6, X7 7); a bit the period does not send gives 0, the erasure of vit_hip_depuncture_batch.
 *     Otherwise di = (k + 1) (n / k) + place, do = di / v, r = di mod v, e = r / (v / 2) + 2 (r mod (v / 2)), q = 126 (do / 126) +
 *     (do mod 126 - s_e) mod 126 with s = (0, 63, 105, 42, 21, 84), out[r][y * steps + n][o] = in[r][y][P(q)][e].  At 2k / QPSK / 1/2 in
 *     an even symbol out[0][1] = in[0][0][0] and out[0][0] = in[0][H(63)][1].
 * Every one of the 2 n_sym steps outputs of every row is written and nothing between the rows; nothing outside the n_sym * Nmax * v
 * elements of a row is read.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the output untouched, for a NULL handle, d_in or d_symbols_out, a handle
 * with R != 2, mode > 2, v not 2, 4 or 6, rate > 4, d_in not aligned to soft_t, d_symbols_out or a parity array not aligned to 4 bytes, at
 * 8-bit symbols an odd out_row_stride with more than one row (every row starts a dword), a non-zero stride below the row, n_sym * Nmax * v,
 * rows or a stride at or above 2^32, an input or output of 2^32 dwords or more, rows * n_sym * Nmax / 504 above 2^31 - 8, an output that
 * overlaps the input or a parity array, d_parity_out overlapping d_parity_in (the same array included) or d_in.  rows = 0 or n_sym = 0
 * returns VIT_HIP_OK with no work (d_parity_out is not written).
 * A batch call like the others: it only enqueues ONE kernel on `stream` (no memset), allocates nothing, needs no workspace, synchronises
 * nothing and can be captured into a hipGraph in front of vit_hip_decode_stream(s).
 * Out of scope: hierarchical modes, the DVB-H in-depth interleaver, OFDM demodulation, pilots, TPS decoding and demapping, DVB-T2, a
 * transmitter on the card. */
int vit_hip_dvbt_deinterleave_batch(vit_hip_handle h, const void* d_in, size_t in_row_stride, size_t rows, size_t n_sym, unsigned mode,
                                    unsigned v, unsigned rate, unsigned parity, const uint32_t* d_parity_in, uint32_t* d_parity_out,
                                    void* d_symbols_out /* [rows][>= n_sym * steps][2] soft_t */, size_t out_row_stride,
                                    vit_hip_stream_t stream);

/* ---- IS-95A forward traffic channel, rate set 1: de-interleave, combine the repetitions, pick the rate ---------------------------------
 * The forward traffic channel of TIA/EIA-95 sends 20 ms frames at 9600, 4800, 2400 or 1200 bit/s through the K = 9, R = 1/2 code, repeats
 * every code symbol 1, 2, 4 or 8 times to 384 symbols, block-interleaves them and scrambles them with the decimated long code -- and sends no
 * rate field.  The receiver combines the repetitions under all four hypotheses, decodes all four and chooses by the frame quality indicator
 * (CRC) and the re-encoded symbol error rate.  These calls stand around vit_hip_decode_batch and vit_hip_crc_batch on a handle of K = 9,
 * R = 2; the de-interleave and the decision do not depend on the polynomials.  The constants are written from memory of TIA/EIA-95
 * 7.1.3; what is stated HERE is the rule.
 * POLYNOMIALS.  In this ABI bit k of a polynomial taps the input of k steps ago.  The stock code "CDMA IS-95A" (491, 369) is 0o753, 0o561
 * read literally under that convention; the standard's figures read with the leftmost bit of 753 on the encoder INPUT -- as 133 / 171 are
 * read for 802.11 -- are the reciprocal set (431, 285) = 0o657, 0o435, which the GENERIC K = 9 kernels serve.
 * Hypothesis h = 0 .. 3, repetition r = 2^h:   rate   bits before the tail L_h   info bits   CRC over the info bits          steps S_h = L_h + 8   bytes
 *                                      h = 0  9600   184                        172         (12, 0xF13, 0xFFF, 0)          192                   23
 *                                      h = 1  4800   88                         80          (8, 0x9B, 0xFF, 0)             96                    11
 *                                      h = 2  2400   40                         40          none                           48                    5
 *                                      h = 3  1200   16                         16          none                           24                    2
 * Transmit side: info bits, the CRC MSB-first (vit_hip_crc_batch's codes), 8 zero tail bits; encoded, c[2 n + o] = polynomial o of step n;
 * repeated, s[q r + j] = c[q] for j < r: 384 symbols at every rate; interleaved, y[i] = s[A(i)] with A(i) = 64 (i mod 6) + BRO6(i div 6),
 * BRO6 the reversal of 6 bits; scrambled, y[i] negated where scramble bit i of the frame is 1.  A(0 .. 7) = 0, 64, 128, 192, 256, 320, 32,
 * 96 (the standard's table, 1-based, starts 1, 65, 129, 193, 257, 321, 33, 97); the inverse is i(a) = 6 BRO6(a mod 64) + a div 64, so s[1] =
 * y[192], s[2] = y[96], s[64] = y[1], s[383] = y[383].
 *
 * vit_hip_is95_deinterleave_batch: descrambles, de-interleaves and combines for the four hypotheses in one launch; soft_t is the handle's
 * symbol type.
 *   - input: frame f is 384 soft_t at d_in + f * in_frame_stride (elements; 0 => 384; a non-zero stride is at least 384);
 *   - d_scramble (may be NULL: nothing is negated): 48 bytes a frame at d_scramble + f * scramble_frame_stride bytes (0 => ONE 48-byte mask
 *     for the whole batch; a non-zero stride is at least 48), bit i of a frame, for received symbol i, being bit 7 - i%8 of byte i/8;
 *   - d_out[h], h = 0 .. 3, any of them NULL but not all: the [frames][S_h][2] buffer vit_hip_decode_batch reads with L = L_h;
 *   - out_h[f][q] = clamp(round_shift(sum over j < 2^h of sg(f, i) in[f][i]), i = i(q 2^h + j)) for q < 2 S_h: sg = -1 where the scramble bit
 *     is set, else +1; int32 arithmetic, -(-32768) is 32768; round_shift(x) = (x + ((1 << shift) >> 1)) >> shift (arithmetic); clamp to
 *     [clamp_lo, clamp_hi] -- the rounding and clamp of vit_hip_lte_rate_dematch_batch.  An erasure (0 where the midpoint of the handle's
 *     soft_decision_high / low is 0) stays one under negation and adds nothing: that is how a caller removes the punctured power-control
 *     symbols.
 * Every element of every non-NULL output is always written; nothing outside a frame's 384 elements and 48 mask bytes is read.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL handle, d_in or d_out, all four outputs
 * NULL, a handle with R != 2, shift > 15, clamp_lo > clamp_hi or either outside soft_t, d_in not aligned to soft_t, an output not aligned to
 * 4 bytes, a non-zero in_frame_stride below 384 or scramble_frame_stride below 48, frames or a stride at or above 2^31 - 1, outputs that
 * overlap each other, the input or the mask.  frames = 0 returns VIT_HIP_OK with no work.
 *
 * vit_hip_is95_channel_errors_batch: for every hypothesis h with d_bytes[h] != NULL, d_errors[h] and d_compared[h] receive exactly what
 * vit_hip_channel_errors_batch(h, d_symbols[h], 0, d_bytes[h], bytes_frame_stride[h], frames, L_h, VIT_HIP_ENCODE_TAIL, NULL, d_errors[h],
 * d_compared[h], stream) writes -- but the up to eight counter arrays are zeroed by ONE kernel of the call's own, not by memsets: 1 + up to
 * 4 launches and no memset node in a captured graph.  Memset nodes of a replayed graph have been seen not to write zeros on this runtime
 * (HISTORY.md, the marker search; with eight of them in one graph the counts of this chain came back wrong from the second replay on), so
 * a chain meant for a graph counts through this call.  Host arrays of four; bytes_frame_stride NULL or an entry 0 => 23, 11, 5, 2.
 * Errors: VIT_HIP_ERR_UNSUPPORTED when vit_hip_info.table_is_linear is 0; VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs
 * untouched, for a NULL handle or array, a handle that is not K = 9, R = 2, all four d_bytes NULL, a present hypothesis without d_symbols,
 * d_errors or d_compared, d_symbols not aligned to soft_t or a count array not to 4 bytes, a non-zero stride that is too small, frames or a
 * stride at or above 2^31 - 1, count arrays that overlap each other or an input.  frames = 0 returns VIT_HIP_OK with no work.
 *
 * vit_hip_is95_rate_decide_batch: the decision and the compaction.  All arrays of pointers and scalars are HOST arrays; what they point to
 * is on the device.
 *   - d_bytes[h]: the decoded bytes of hypothesis h, frame f at d_bytes[h] + f * bytes_frame_stride[h] (bytes_frame_stride NULL or an entry
 *     0 => 23, 11, 5, 2; a non-zero stride is at least that), bit t of a frame being bit 7 - t%8 of byte t/8.  NULL takes hypothesis h out
 *     of the contest; not all four;
 *   - d_errors[h], d_compared[h], uint32 [frames]: what vit_hip_channel_errors_batch wrote for d_out[h] and d_bytes[h] with L = L_h and
 *     VIT_HIP_ENCODE_TAIL; d_syndrome[0], d_syndrome[1], uint32 [frames]: what vit_hip_crc_batch wrote with rows = 1, first_bit = 0, n_bits =
 *     172 / 80 and the codes above.  Required for a present hypothesis, not read for an absent one;
 *   - hypothesis h PASSES for frame f when it is present, h >= 2 or its syndrome is 0, compared_h > 0 and errors_h * ser_den <= compared_h *
 *     max_ser_num[h] (64-bit products; ser_den > 0).  rate = the passing h with the smallest errors_h / compared_h, compared by 64-bit
 *     cross-multiplication, the lower h on a tie; 4 where nothing passes: an erased frame.  A transparent default, not a policy: the
 *     standard prescribes no rule and every input stays with the caller;
 *   - d_decision[f] = {rate, info_bits (172, 80, 40, 16; 0 at rate 4), errors, compared of the winner (0 at rate 4)};
 *   - d_info + f * info_stride (0 => 22; a non-zero stride is at least 22): all 22 bytes are always written; the first info_bits bits are
 *     those of the winner's bytes, every bit behind them is 0 -- byte 21 of a full-rate frame keeps its top 4 bits.
 * Whatever the count and syndrome memory holds, nothing outside the frames' own bytes and entries is read.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL handle, array, d_decision or d_info, all
 * four d_bytes NULL, a present hypothesis without its counts (or, h < 2, its syndrome), ser_den = 0, a non-zero stride that is too small,
 * d_decision or a count array not aligned to 4 bytes, frames or a stride at or above 2^31 - 1, an output that overlaps the other or an
 * input.  frames = 0 returns VIT_HIP_OK with no work.
 * Batch calls like the others: the de-interleave and the decision each enqueue ONE kernel on `stream`, the error counts up to five, none a
 * memset; they allocate nothing, need no workspace, synchronise nothing, read the handle only for its device, soft_t, K and R (the error
 * counts: its polynomials too), and can be captured into a hipGraph: de-interleave, 4 decodes, the error counts, 2 CRCs and the decision
 * are one graph.
 * Out of scope: rate set 2 (14400 and its puncturing); the long-code generator itself (the caller supplies the decimated bits);
 * power-control bit extraction; sync and paging channels (continuous encoding: vit_hip_decode_stream); the reverse link (other interleaver,
 * 64-ary orthogonal modulation); cdma2000 radio configurations 3 and up (R = 1/4 with puncturing); any rate-decision policy beyond the
 * rule above. */
typedef struct vit_hip_is95_decision { uint32_t rate, info_bits, errors, compared; } vit_hip_is95_decision;
int vit_hip_is95_deinterleave_batch(vit_hip_handle h, const void* d_in, size_t in_frame_stride, size_t frames, const uint8_t* d_scramble,
                                    size_t scramble_frame_stride, unsigned shift, int clamp_lo, int clamp_hi,
                                    void* const d_out[4] /* [frames][S_h][2] soft_t each, or NULL */, vit_hip_stream_t stream);
int vit_hip_is95_channel_errors_batch(vit_hip_handle h, const void* const d_symbols[4], const uint8_t* const d_bytes[4],
                                      const size_t bytes_frame_stride[4], size_t frames, uint32_t* const d_errors[4],
                                      uint32_t* const d_compared[4], vit_hip_stream_t stream);
int vit_hip_is95_rate_decide_batch(vit_hip_handle h, const uint8_t* const d_bytes[4], const size_t bytes_frame_stride[4],
                                   const uint32_t* const d_errors[4], const uint32_t* const d_compared[4],
                                   const uint32_t* const d_syndrome[2], size_t frames, const uint32_t max_ser_num[4], uint32_t ser_den,
                                   vit_hip_is95_decision* d_decision, uint8_t* d_info, size_t info_stride, vit_hip_stream_t stream);

/* ---- GSM channel decoding: burst de-interleaver, the Fire code of the control channels, TCH/FS frames -----------------------------------
 * GSM (3GPP TS 45.003, formerly GSM 05.03) protects its control channels (SACCH, BCCH, CCCH, SDCCH, FACCH; the CS-1 layout) and full-rate
 * speech (TCH/FS) with the K = 5, R = 1/2 code G0 = 1 + D^3 + D^4, G1 = 1 + D + D^3 + D^4 and spreads a block of 456 coded bits over the
 * 114 payload bits of 4 or 8 bursts.  These calls stand around vit_hip_decode_batch on a handle of K = 5, R = 2; none of them depends on the
 * polynomials.  The constants are written from memory of TS 45.003 clauses 3.1, 4.1 and 4.3; what is stated HERE is the rule.
 * POLYNOMIALS.  In this ABI bit k of a polynomial taps the input of k steps ago: the GSM code is (25, 27) = (0b11001, 0b11011), not the
 * stock "Basic K=5 R=1/2" (23, 25); the input bits 1 0 0 0 0 encode to the pairs 11 01 00 11 11.  The GENERIC K = 5 kernels serve it.
 *
 * vit_hip_gsm_deinterleave_batch: bursts -> the symbols vit_hip_decode_batch reads; soft_t is the handle's symbol type.
 *   - input: `rows` rows of `bursts` bursts, one row per logical channel: burst B of row r is the 116 soft_t e(B, 0 .. 115) at d_in + r *
 *     in_row_stride + B * in_burst_stride (elements; in_burst_stride 0 => 116, in_row_stride 0 => bursts * the burst stride), the two
 *     half-bursts of 57 with the stealing flags hl = e(B, 57) and hu = e(B, 58) between them.  bursts is a multiple of 4 = 4 m;
 *   - flags VIT_HIP_GSM_NEGATE: every value read from d_in or d_hist_in is negated on the way, in int32, and clamped to the range of soft_t
 *     (-(-128) is 127): for demodulators that send bit 1 as the negative value, or a caller who folds the A5 keystream into the sign
 *     beforehand.  An erasure at a midpoint of 0 stays one;
 *   - the map: coded bit k = 0 .. 455 of block n is payload position j(k) = 2 ((49 k) mod 57) + ((k mod 8) div 4) of burst B, read as
 *     e(B, j) for j < 57 and e(B, j + 2) for j >= 57.  j(0 .. 7) = 0, 98, 82, 66, 51, 35, 19, 3.
 *     mode VIT_HIP_GSM_BLOCK: B = 4 n + (k mod 4); a bijection onto 4 x 114; no history; every row gives m blocks.
 *     mode VIT_HIP_GSM_DIAGONAL (TCH/F, FACCH/F): B = 4 n + (k mod 8) in the SEQUENCE of the row: the four bursts of d_hist_in + r * 464
 *     where d_hist_in is given and d_fill_in[r] == 4, then the input.  The first four bursts of a block carry its even j, the last four
 *     its odd j, 57 each.  A row with history gives m blocks, one without m - 1, compacted to the front of the row's m slots; the slots
 *     behind them are written as zeros (d_steal too), so every byte of every output is defined;
 *   - the carried state, diagonal mode only: d_hist_out + r * 464 receives the last four bursts of the row's input AS RECEIVED (not
 *     negated; a call with the flag negates them when it reads them) and d_fill_out[r] = 4.  d_hist_in / d_fill_in and d_hist_out /
 *     d_fill_out come in pairs, each pair may be NULL, and they travel between two sets of arrays from call to call like the history of
 *     vit_hip_dab_deinterleave_batch, so a captured graph of two calls replays correctly.  d_fill_in[r] other than 4 means no history;
 *   - d_n_out (may be NULL), uint32 [rows]: the blocks row r gave: m, or m - 1;
 *   - outputs, any of them NULL but not all four: d_full [rows][m][228][2] soft_t, coded bit k at [k / 2][k % 2]: what the decode reads with
 *     L = 224 (xCCH, FACCH: 184 data + 40 parity bits, 4 tail bits); d_class1 [rows][m][189][2], coded bits 0 .. 377: with L = 185 (TCH/FS);
 *     d_class2 [rows][m][78], coded bits 378 .. 455; d_steal int32 [rows][m]: the sum of the block's stealing flags after the optional
 *     negation -- hu of the first four bursts plus hl of the last four in diagonal mode, all eight flags of the four bursts in block mode.
 *     The caller thresholds it to tell FACCH from speech.
 * Nothing outside the 116 elements of a burst and the 464 of a row's history is read.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL handle or d_in, d_full, d_class1, d_class2
 * and d_steal all NULL, a handle with R != 2, mode above VIT_HIP_GSM_DIAGONAL, flags other than VIT_HIP_GSM_NEGATE, any of the four history
 * arguments in block mode, d_hist_in without d_fill_in or d_hist_out without d_fill_out (and the reverse), bursts no multiple of 4, a
 * symbol buffer not aligned to soft_t, a count array or d_steal not aligned to 4 bytes, a non-zero in_burst_stride below 116 or
 * in_row_stride below a row's bursts, rows, bursts, rows * m or a stride at or above 2^31 - 1, an output (d_hist_out, d_fill_out and d_n_out
 * included) that overlaps another or d_in, d_hist_in or d_fill_in.  rows = 0 or bursts = 0 returns VIT_HIP_OK with no work.
 *
 * vit_hip_gsm_fire_batch: the Fire code (224, 184) of the control channels, g(D) = (D^23 + 1)(D^17 + D^3 + 1) = D^40 + D^26 + D^23 + D^17 +
 * D^3 + 1 = 0x10004820009.
 *   - input: frame f is the 28 bytes at d_bytes + f * bytes_frame_stride (0 => 28), bit u(t), t = 0 .. 223, being bit 7 - t%8 of byte t/8 as
 *     vit_hip_decode_batch writes them with L = 224: the 184 data bits d first, then the 40 parity bits;
 *   - syndrome = (r mod g) XOR (2^40 - 1) with r(D) = sum of u(t) D^(223 - t): the standard makes the remainder all ones.  184 zero data
 *     bits carry 40 parity ones; an error in u(223) alone gives syndrome 1, one in u(183) alone 0x0004820009;
 *   - max_burst = 0 .. 12 (0: detect only).  Syndrome 0: status 0.  Otherwise the call looks for THE error pattern p(D) D^m with p(0) = 1,
 *     deg p < max_burst, m >= 0 and m + deg p <= 223 whose remainder mod g is the syndrome: p = syndrome D^(-m) mod g.  All 438 271 patterns
 *     of length <= 12 inside 224 bits have distinct non-zero syndromes, so there is at most one.  Found: its bits are flipped, status = deg
 *     p + 1 (the burst's length), first_bit = 223 - m - deg p (the first flipped t).  Not found: status = -1, first_bit = 0 and the bits go
 *     out as received.  A frame with more errors than one burst may be "corrected" to another codeword: the code's limit, not the call's;
 *   - d_status[f] = {status, first_bit, syndrome_lo, syndrome_hi}: the syndrome as received, bits 0 .. 31 and 32 .. 39;
 *   - d_data + f * data_stride (0 => 23): the 23 data bytes, d(8 i + b) as bit 7 - b of byte i -- or, with VIT_HIP_GSM_LSB_FIRST, as bit b,
 *     the octet order of GSM 04.04.  In place is allowed: d_data == d_bytes with the same (resolved) stride.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL handle, d_bytes, d_status or d_data,
 * max_burst above 12, flags other than VIT_HIP_GSM_LSB_FIRST, d_status not aligned to 4 bytes, a non-zero bytes_frame_stride below 28 or
 * data_stride below 23, frames or a stride at or above 2^31 - 1, d_status overlapping d_bytes or d_data, d_data overlapping d_bytes other
 * than in place.  frames = 0 returns VIT_HIP_OK with no work.
 *
 * vit_hip_gsm_tchfs_batch: decoded class I bits and class II soft bits -> 260-bit speech frames.
 *   - input: frame f is the 24 bytes at d_bytes + f * bytes_frame_stride (0 => 24), u(0 .. 184) as vit_hip_decode_batch writes them with L =
 *     185, and the 78 soft_t at d_class2 + f * 78, what the de-interleaver wrote;
 *   - d(2 k) = u(k) and d(2 k + 1) = u(184 - k) for k = 0 .. 90; p(k) = u(91 + k), k = 0, 1, 2; d(182 + k) = 1 where 2 c > high + low for
 *     class II value c = d_class2[f][k] and the handle's soft_decision_high / low, the rule of vit_hip_channel_errors_batch; a value at the
 *     midpoint gives 0 and is counted;
 *   - d_speech + f * speech_stride (0 => 33): 33 bytes, d(t) as bit 7 - t%8 of byte t/8, the last four bits 0;
 *   - d_status[f] (d_status may be NULL) = {parity_syndrome, class2_erasures}: the 3 bits (d(0 .. 49) D^3 + p(0) D^2 + p(1) D + p(2)) mod (D^3 +
 *     D + 1), XORed with 7 -- 0 where the parity holds: vit_hip_crc_batch's (3, 0x3, 0, 0x7) over d(0 .. 49) --, and the class II values at
 *     the midpoint.
 * Errors: VIT_HIP_ERR_INVALID_ARG, with nothing launched and the outputs untouched, for a NULL handle, d_bytes, d_class2 or d_speech,
 * d_class2 not aligned to soft_t or d_status to 4 bytes, a non-zero bytes_frame_stride below 24 or speech_stride below 33, frames or a stride
 * at or above 2^31 - 1, an output that overlaps an input or the other output.  frames = 0 returns VIT_HIP_OK with no work.
 * Batch calls like the others: each enqueues ONE kernel on `stream` and no memset (memset nodes of a replayed graph have produced wrong
 * counts on this runtime: see the IS-95 error counts above), allocates nothing, needs no workspace, synchronises nothing, always writes
 * every element of every non-NULL output and can be captured into a hipGraph: de-interleave, decode, Fire is the control-channel
 * receiver, de-interleave, two decodes, TCH/FS and Fire the TCH/F one.
 * Out of scope: GPRS CS-2..4 and EGPRS (puncturing tables, USF precoding); TCH/HS, EFR's preliminary CRC-8, AMR; SACCH/TCH multiframe
 * scheduling and deciphering (the caller negates with the A5 keystream); burst demodulation; per-row burst counts in one call; a
 * transmitter on the card.  SCH, RACH and the TCH/FS parity alone need no call of their own: vit_hip_crc_batch with (10, 0x175, 0, 0x3FF),
 * (6, 0x2F, 0, 0x3F) -- the syndrome is the BSIC -- and (3, 0x3, 0, 0x7). */
#define VIT_HIP_GSM_BLOCK 0u
#define VIT_HIP_GSM_DIAGONAL 1u
#define VIT_HIP_GSM_NEGATE 1u       /* flags of vit_hip_gsm_deinterleave_batch */
#define VIT_HIP_GSM_LSB_FIRST 1u    /* flags of vit_hip_gsm_fire_batch */
typedef struct vit_hip_gsm_fire { int32_t status; uint32_t first_bit, syndrome_lo, syndrome_hi; } vit_hip_gsm_fire;
typedef struct vit_hip_gsm_tchfs { uint32_t parity_syndrome, class2_erasures; } vit_hip_gsm_tchfs;
int vit_hip_gsm_deinterleave_batch(vit_hip_handle h, const void* d_in, size_t in_row_stride, size_t in_burst_stride, size_t rows, size_t bursts,
                                   unsigned mode, unsigned flags, const void* d_hist_in, const uint32_t* d_fill_in, void* d_hist_out,
                                   uint32_t* d_fill_out, uint32_t* d_n_out, void* d_full /* [rows][bursts / 4][228][2] soft_t, or NULL */,
                                   void* d_class1 /* [rows][bursts / 4][189][2] */, void* d_class2 /* [rows][bursts / 4][78] */,
                                   int32_t* d_steal /* [rows][bursts / 4] */, vit_hip_stream_t stream);
int vit_hip_gsm_fire_batch(vit_hip_handle h, const uint8_t* d_bytes, size_t bytes_frame_stride, size_t frames, unsigned max_burst,
                           unsigned flags, vit_hip_gsm_fire* d_status, uint8_t* d_data, size_t data_stride, vit_hip_stream_t stream);
int vit_hip_gsm_tchfs_batch(vit_hip_handle h, const uint8_t* d_bytes, size_t bytes_frame_stride, const void* d_class2, size_t frames,
                            uint8_t* d_speech, size_t speech_stride, vit_hip_gsm_tchfs* d_status, vit_hip_stream_t stream);

/* The clock the SIMDs sustain under the update kernels' instruction class, measured on the device: every SIMD runs four waves
 * of independent v_pk_add_u16 for about 2 ms between readings of s_memtime (shader clocks) and s_memrealtime (constant
 * reference clock); *mhz_out = their median ratio x the reference rate.  *cycles_per_pk_instr_out (may be NULL) = shader
 * clocks one SIMD needed per wave64 packed instruction in that loop.  With cycles_per_pk_instr_out == NULL the probe is ONE
 * wave per CU: light enough to read the clock WHILE other kernels run (launched on the null stream; the decode pipeline's
 * streams are non-blocking) without adding a chip full of vector work to their power draw.  Synchronous; measurement harness
 * (bench.py quotes its VALU ceiling at this clock, not at a nominal one). */
int vit_hip_shader_clock_mhz(int device, double* mhz_out, double* cycles_per_pk_instr_out);

/* ---- host-pointer compatibility route (one decoder object, streaming) ------------------------------------------ */

/* update() on a host-resident decoder state: metrics_inout [N] error_t ("old" metrics), symbols n_steps*R soft_t,
 * decisions_out [n_steps][W] (rows for THIS call), *renorm_sum_out = update()'s return value.  Synchronous. */
int vit_hip_update_host(vit_hip_handle h, void* metrics_inout, const void* symbols, size_t n_steps,
                        uint64_t* decisions_out, uint64_t* renorm_sum_out);

/* chainback() on host-resident rows: decisions [L+K-1][W].  Synchronous. */
int vit_hip_chainback_host(vit_hip_handle h, const uint64_t* decisions, size_t L, size_t end_state, uint8_t* bytes_out);

/* ---- the FRAME route of the header-level drop-in: update() and the chainback() behind it in ONE launch ---------------------------
 * vit_hip_update_host / vit_hip_chainback_host above keep the reference's division of labour -- every call hands the decision rows
 * back to the host and takes them in again (core.h:214-236 reads m_decisions on the host) -- which for one frame means two launches,
 * two synchronisations and four staging copies around 0.3 ms of trellis.  The lazy pair leaves the rows where they were made:
 *   vit_hip_update_host_lazy    runs n_steps steps like vit_hip_update_host, but stores their decision rows as rows [first_row,
 *       first_row + n_steps) of the handle's DEVICE row store instead of returning them (the store keeps earlier rows; a handle has
 *       one frame's rows, as a ViterbiDecoder_Core has one m_decisions).  K <= 7 (and K = 8, 9 with R <= 4): symbols are read straight from pinned host-mapped
 *       memory, metrics / renormalisation sum come back through it, and the host polls a completion word instead of synchronising
 *       the stream.  When the call COMPLETES a frame of `speculate_bits` decoded bits (first_row + n_steps == speculate_bits + K-1;
 *       0 = never) the same launch also chains back those bits from `speculate_end_state` and keeps the bytes;
 *   vit_hip_chainback_host_lazy chainback(L, end_state) over the device row store: the bytes kept by the completing update if it was
 *       asked for exactly this (L, end_state) and no other lazy update ran since -- no GPU work at all -- else one kernel;
 *   vit_hip_fetch_decisions_host  copies rows of the device row store to the host (what reading m_decisions[row] triggers).
 * The caller tracks which rows are authoritative where (include/viterbi_hip/viterbi_decoder_core.h does): rows written by
 * vit_hip_update_host_lazy live on the device until fetched; rows the caller changed on the host make it use the eager pair again. */
int vit_hip_update_host_lazy(vit_hip_handle h, void* metrics_inout, const void* symbols, size_t n_steps, size_t first_row,
                             size_t speculate_bits, size_t speculate_end_state, uint64_t* renorm_sum_out);
int vit_hip_chainback_host_lazy(vit_hip_handle h, size_t L, size_t end_state, uint8_t* bytes_out);
int vit_hip_fetch_decisions_host(vit_hip_handle h, size_t first_row, size_t n_rows, uint64_t* decisions_out);

/* Which kernels serve the single-decoder routes above (eager pair and frame route alike) for this handle's (K, R):
 *   "single-frame in-place (K = 7)"   K = 7, R <= 4: one wavefront walks the trellis in place, two helper wavefronts beside it
 *   "single-frame lane == state"      K <= 7, R <= 8 otherwise: one wavefront, one state per lane
 *   "single-frame wide (K = 8, 9)"    K = 8, 9 with R <= 4: one wavefront, lane == state mod 64, two or four states per lane
 *   "PLAN_LDS on one frame"           everything else (R >= 5 at K = 8, 9; K >= 10): the general LDS kernels, two workgroup barriers
 *                                     per trellis step -- the note says which limit the code is beyond
 * VIT_HIP_HOST_ROUTE_LDS forces the last family at any K (results are bit for bit those of the others: an A/B inside one process);
 * VIT_HIP_HOST_ROUTE_AUTO (the default) gives the choice back.  Rows already in the device row store stay valid across a change.
 * The note is one line of text in thread-local storage, valid until the thread's next call, like vit_hip_plan_note's. */
#define VIT_HIP_HOST_ROUTE_AUTO 0
#define VIT_HIP_HOST_ROUTE_LDS 1
const char* vit_hip_host_route_note(vit_hip_handle h);
int vit_hip_set_host_route(vit_hip_handle h, int route);

#ifdef __cplusplus
}
#endif
#endif /* VIT_HIP_H */
