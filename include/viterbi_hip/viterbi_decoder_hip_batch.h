// viterbi_hip/viterbi_decoder_hip_batch.h -- RAII wrapper over the batched C ABI (include/vit_hip.h): many independent
// frames, buffers resident in HBM, explicit stream.  Built from the same host types as the single-frame drop-in
// (ViterbiBranchTable, ViterbiDecoder_Config), so a program moves from
//     for each frame: vitdec.reset(); Decoder::update(vitdec, ...); vitdec.chainback(...)      (examples/run_benchmark.cpp:268-281)
// to one call per batch without touching how the code or the configuration is described.  No HIP header is needed here:
// device pointers and the stream are passed as plain pointers; allocation stays with the caller.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../vit_hip.h"
#include "viterbi_branch_table.h"
#include "viterbi_decoder_config.h"

template <size_t constraint_length, size_t code_rate, typename error_t, typename soft_t>
class ViterbiDecoder_HIP_Batch {
public:
    static constexpr size_t K = constraint_length, R = code_rate;
    static constexpr size_t NUMSTATES = size_t(1) << (K - 1);
    using BranchTable = ViterbiBranchTable<K, R, soft_t>;
    using Config = ViterbiDecoder_Config<error_t>;

    ViterbiDecoder_HIP_Batch(const BranchTable& table, const Config& config, int device = 0) {
        check(vit_hip_create(int(K), int(R), int(sizeof(soft_t)), int(sizeof(error_t)), table.data(), &config, device, &m_hip),
              "vit_hip_create");
    }
    ~ViterbiDecoder_HIP_Batch() { vit_hip_destroy(m_hip); }
    ViterbiDecoder_HIP_Batch(const ViterbiDecoder_HIP_Batch&) = delete;
    ViterbiDecoder_HIP_Batch& operator=(const ViterbiDecoder_HIP_Batch&) = delete;

    // bytes of device workspace (256-byte aligned) the decision history of `frames` frames of `total_bits` bits needs
    size_t workspace_bytes(size_t frames, size_t total_bits) const { return vit_hip_workspace_bytes(m_hip, frames, total_bits); }
    static size_t symbols_per_frame(size_t total_bits) { return (total_bits + K - 1) * R; }

    // reset -> update -> chainback for every frame; everything is enqueued on `stream` (a hipStream_t), nothing synchronises
    void decode(const soft_t* d_symbols, size_t frames, size_t total_bits, void* d_workspace, size_t workspace_size,
                uint8_t* d_bytes_out, error_t* d_final_metrics = nullptr, uint64_t* d_renorm_sum = nullptr,
                const uint32_t* d_end_state = nullptr, void* stream = nullptr) {
        check(vit_hip_decode_batch(m_hip, d_symbols, frames, total_bits, d_workspace, workspace_size, d_bytes_out,
                                   d_final_metrics, d_renorm_sum, d_end_state, stream), "vit_hip_decode_batch");
    }
    // the two phases separately, as the reference times them (run_benchmark.cpp:272-281)
    void update(const soft_t* d_symbols, size_t frames, size_t total_bits, void* d_workspace, size_t workspace_size,
                error_t* d_final_metrics = nullptr, uint64_t* d_renorm_sum = nullptr, const uint32_t* d_start_state = nullptr,
                void* stream = nullptr) {
        check(vit_hip_update_batch(m_hip, d_symbols, frames, total_bits + K - 1, total_bits, d_workspace, workspace_size,
                                   d_final_metrics, d_renorm_sum, d_start_state, stream), "vit_hip_update_batch");
    }
    void chainback(const void* d_workspace, size_t frames, size_t total_bits, uint8_t* d_bytes_out,
                   const uint32_t* d_end_state = nullptr, void* stream = nullptr) {
        check(vit_hip_chainback_batch(m_hip, d_workspace, frames, total_bits, d_bytes_out, d_end_state, stream),
              "vit_hip_chainback_batch");
    }
    // depuncturing front-end (examples/helpers/puncture_code_helpers.h:17-55 for a batch): d_source_index[k] is the position of
    // mother-code symbol k among the `punctured_per_frame` transmitted ones, or < 0 for a punctured symbol (erasure value 0)
    void depuncture(const soft_t* d_punctured, size_t punctured_per_frame, const int32_t* d_source_index, size_t frames,
                    size_t total_bits, soft_t* d_symbols_out, void* stream = nullptr) {
        check(vit_hip_depuncture_batch(m_hip, d_punctured, punctured_per_frame, d_source_index, symbols_per_frame(total_bits),
                                       frames, d_symbols_out, stream), "vit_hip_depuncture_batch");
    }
    // batched streaming: decoders that keep their state on the device between calls (the reference's update() cursor,
    // viterbi_decoder_scalar.h:37-54): reset() once, then resume() over consecutive step ranges, then chainback()
    void reset(size_t frames, error_t* d_metrics, const uint32_t* d_start_state = nullptr, void* stream = nullptr) {
        check(vit_hip_reset_batch(m_hip, frames, d_start_state, d_metrics, stream), "vit_hip_reset_batch");
    }
    void resume(const soft_t* d_symbols, size_t symbol_frame_stride, size_t frames, size_t first_step, size_t n_steps,
                size_t total_bits, void* d_workspace, size_t workspace_size, error_t* d_metrics_inout,
                uint64_t* d_renorm_sum = nullptr, void* stream = nullptr) {
        check(vit_hip_update_batch_resume(m_hip, d_symbols, symbol_frame_stride, frames, first_step, n_steps, total_bits,
                                          d_workspace, workspace_size, d_metrics_inout, d_renorm_sum, stream),
              "vit_hip_update_batch_resume");
    }
    // tail-biting frames (vit_hip_decode_tail_biting_batch): d_symbols [frames][total_bits][R], no tail; wrap-around Viterbi with
    // `head` steps of extension before the frame and `tail` after it (0: the default 8*(K-1)).  The workspace is caller-owned.
    size_t tail_biting_workspace_bytes(size_t frames, size_t total_bits, size_t head = 0, size_t tail = 0) const {
        return vit_hip_tail_biting_workspace_bytes(m_hip, frames, total_bits, extension(head), extension(tail));
    }
    void decode_tail_biting(const soft_t* d_symbols, size_t frames, size_t total_bits, void* d_workspace, size_t workspace_size,
                            uint8_t* d_bytes_out, uint32_t* d_end_state_out = nullptr, uint8_t* d_tail_biting_ok = nullptr,
                            size_t head = 0, size_t tail = 0, void* stream = nullptr) {
        check(vit_hip_decode_tail_biting_batch(m_hip, d_symbols, frames, total_bits, extension(head), extension(tail), d_workspace,
                                               workspace_size, d_bytes_out, d_end_state_out, d_tail_biting_ok, stream),
              "vit_hip_decode_tail_biting_batch");
    }
    // one long unterminated stream (vit_hip_decode_stream): d_symbols [steps][R], one segment per call, decoded as overlapped
    // windows of `window` steps (0: 1024) with `head` steps of lead-in and `tail` of look-ahead (0: the default 8*(K-1)); begin /
    // end: the segment holds the encoder's start / the zero tail.  Returns the number of bits written to d_bytes_out, MSB-first.
    size_t stream_workspace_bytes(size_t steps, bool begin, bool end, size_t window = 0, size_t head = 0, size_t tail = 0) const {
        return vit_hip_stream_workspace_bytes(m_hip, steps, window_or_default(window), extension(head), extension(tail),
                                              stream_flags(begin, end));
    }
    size_t decode_stream(const soft_t* d_symbols, size_t steps, bool begin, bool end, void* d_workspace, size_t workspace_size,
                         uint8_t* d_bytes_out, size_t window = 0, size_t head = 0, size_t tail = 0, void* stream = nullptr) {
        size_t n_bits = 0;
        check(vit_hip_decode_stream(m_hip, d_symbols, steps, window_or_default(window), extension(head), extension(tail),
                                    stream_flags(begin, end), d_workspace, workspace_size, d_bytes_out, &n_bits, stream),
              "vit_hip_decode_stream");
        return n_bits;
    }
    // n_streams lockstep streams in one call on one shared window grid (vit_hip_decode_streams): d_symbols [n_streams][pitch][R],
    // stream s in steps [s*pitch, s*pitch + steps), pitch a multiple of the window; row s of d_bytes_out [n_streams][out_pitch_bytes]
    // is what decode_stream returns for stream s.  Defaults as decode_stream.  Returns the number of bits written to each row.
    size_t streams_workspace_bytes(size_t n_streams, size_t pitch, size_t steps, bool begin, bool end, size_t window = 0,
                                   size_t head = 0, size_t tail = 0) const {
        return vit_hip_streams_workspace_bytes(m_hip, n_streams, pitch, steps, window_or_default(window), extension(head), extension(tail),
                                               stream_flags(begin, end));
    }
    size_t decode_streams(const soft_t* d_symbols, size_t n_streams, size_t pitch, size_t steps, bool begin, bool end, void* d_workspace,
                          size_t workspace_size, uint8_t* d_bytes_out, size_t out_pitch_bytes, size_t window = 0, size_t head = 0,
                          size_t tail = 0, void* stream = nullptr) {
        size_t n_bits = 0;
        check(vit_hip_decode_streams(m_hip, d_symbols, n_streams, pitch, steps, window_or_default(window), extension(head), extension(tail),
                                     stream_flags(begin, end), d_workspace, workspace_size, d_bytes_out, out_pitch_bytes, &n_bits,
                                     stream),
              "vit_hip_decode_streams");
        return n_bits;
    }
    // test / measurement harness on the device: the BER harness's frame generator (examples/run_snr_ber.cpp:311-359) and
    // get_total_bit_errors (examples/helpers/test_helpers.h:95-104)
    void synth(size_t frames, size_t total_bits, uint64_t seed, uint64_t first_frame, float ebn0_db, bool noise_free,
               uint8_t* d_tx_bytes, soft_t* d_symbols, void* stream = nullptr) {
        check(vit_hip_synth_batch(m_hip, frames, total_bits, seed, first_frame, ebn0_db, noise_free ? 1 : 0, d_tx_bytes,
                                  d_symbols, stream), "vit_hip_synth_batch");
    }
    void count_bit_errors(const uint8_t* d_a, const uint8_t* d_b, size_t n_bytes, uint64_t* d_count, void* stream = nullptr) {
        check(vit_hip_count_bit_errors(m_hip, d_a, d_b, n_bytes, d_count, stream), "vit_hip_count_bit_errors");
    }
    // the encoder on the caller's own bytes (vit_hip_encode_batch) and the re-encoded channel symbol error count of decoded bytes
    // against the received symbols (vit_hip_channel_errors_batch): flags VIT_HIP_ENCODE_TAIL / _TAIL_BITING or 0 (a piece of a
    // stream), strides in elements (0: packed), states in the decoder's numbering; d_errors / d_compared [frames] are overwritten
    void encode(const uint8_t* d_bytes, size_t frames, size_t total_bits, soft_t* d_symbols_out, unsigned flags = VIT_HIP_ENCODE_TAIL,
                const uint32_t* d_start_state = nullptr, uint32_t* d_end_state_out = nullptr, size_t bytes_frame_stride = 0,
                size_t symbol_frame_stride = 0, void* stream = nullptr) {
        check(vit_hip_encode_batch(m_hip, d_bytes, bytes_frame_stride, frames, total_bits, flags, d_start_state, d_symbols_out,
                                   symbol_frame_stride, d_end_state_out, stream), "vit_hip_encode_batch");
    }
    void channel_errors(const soft_t* d_symbols, const uint8_t* d_bytes, size_t frames, size_t total_bits, uint32_t* d_errors,
                        uint32_t* d_compared = nullptr, unsigned flags = VIT_HIP_ENCODE_TAIL, const uint32_t* d_start_state = nullptr,
                        size_t symbol_frame_stride = 0, size_t bytes_frame_stride = 0, void* stream = nullptr) {
        check(vit_hip_channel_errors_batch(m_hip, d_symbols, symbol_frame_stride, d_bytes, bytes_frame_stride, frames, total_bits,
                                           flags, d_start_state, d_errors, d_compared, stream), "vit_hip_channel_errors_batch");
    }
    // node synchronisation (vit_hip_sync_build / vit_hip_sync_search): the [steps][R] streams of up to 64 alignment hypotheses (a HOST
    // array of {offset, VIT_HIP_SYNC_* flags}) from one received buffer -- d_source_index / period_symbols / kept_per_period describe
    // ONE puncturing period as for depuncture(), nullptr / 0 / 0 = unpunctured -- and their ranking by the re-encoded channel symbol
    // error count in one call: d_errors / d_compared [n_hyp] and d_best [1] (may be nullptr) are the results.  window / head / tail as
    // decode_streams (0: the defaults); pitch in steps (0: `steps`).  The workspace is caller-owned.
    void sync_build(const soft_t* d_received, size_t n_received, const int32_t* d_source_index, size_t period_symbols,
                    size_t kept_per_period, const vit_hip_sync_hypothesis* hypotheses, size_t n_hyp, size_t steps,
                    soft_t* d_symbols_out, size_t pitch = 0, void* stream = nullptr) {
        check(vit_hip_sync_build(m_hip, d_received, n_received, d_source_index, period_symbols, kept_per_period, hypotheses, n_hyp, steps,
                                 pitch ? pitch : steps, d_symbols_out, stream), "vit_hip_sync_build");
    }
    size_t sync_search_workspace_bytes(size_t n_hyp, size_t steps, size_t window = 0, size_t head = 0, size_t tail = 0) const {
        return vit_hip_sync_search_workspace_bytes(m_hip, n_hyp, steps, window_or_default(window), extension(head), extension(tail));
    }
    void sync_search(const soft_t* d_received, size_t n_received, const int32_t* d_source_index, size_t period_symbols,
                     size_t kept_per_period, const vit_hip_sync_hypothesis* hypotheses, size_t n_hyp, size_t steps, void* d_workspace,
                     size_t workspace_size, uint32_t* d_errors, uint32_t* d_compared, uint32_t* d_best = nullptr, size_t window = 0,
                     size_t head = 0, size_t tail = 0, void* stream = nullptr) {
        check(vit_hip_sync_search(m_hip, d_received, n_received, d_source_index, period_symbols, kept_per_period, hypotheses, n_hyp, steps,
                                  window_or_default(window), extension(head), extension(tail), d_workspace, workspace_size, d_errors,
                                  d_compared, d_best, stream), "vit_hip_sync_search");
    }
    // frame synchronisation (vit_hip_marker_search): the distance of a sync marker of marker_bits <= 64 bits to every bit position of
    // rows of decoded bytes (MSB-first; bytes_row_stride 0: packed), summed per phase (phase0 + position) mod period_bits into
    // d_distance / d_count [rows][period_bits] (d_count may be nullptr), and into d_lock [rows] (may be nullptr) the phase and
    // polarity no other beats.  d_history [rows] holds the history_bits <= 63 stream bits in front of bit 0 of each row, the latest in
    // bit 0.  flags: 0 overwrites the totals, VIT_HIP_MARKER_ACCUMULATE adds to them (a receiver's running totals).
    void marker_search(const uint8_t* d_bytes, size_t rows, size_t n_bits, uint64_t marker, unsigned marker_bits, size_t period_bits,
                       uint32_t* d_distance, uint32_t* d_count = nullptr, vit_hip_marker_lock* d_lock = nullptr, size_t phase0 = 0,
                       const uint64_t* d_history = nullptr, unsigned history_bits = 0, unsigned flags = 0, size_t bytes_row_stride = 0,
                       void* stream = nullptr) {
        check(vit_hip_marker_search(m_hip, d_bytes, bytes_row_stride, rows, n_bits, marker, marker_bits, d_history, history_bits,
                                    period_bits, phase0, flags, d_distance, d_count, d_lock, stream), "vit_hip_marker_search");
    }
    // frame extraction (vit_hip_frames_extract): the frames of rows of decoded bytes cut at the lock marker_search wrote (d_lock, read on
    // the device), each from bit 0 of a byte on at d_frames + (row * max_frames + f) * frame_stride_bytes: complemented under an
    // inverted lock, the first drop_bits bits (the marker) dropped, d_pad [ceil((period_bits - drop_bits) / 8)] (the randomiser; may be
    // nullptr) XORed off.  d_n_frames [rows] receives the frames completed, d_marker_errors [rows][max_frames] (may be nullptr, with
    // marker_bits 0: off) the marker bits of each that differ, d_carry_out / d_carry_bits_out the unfinished frame's raw bits, which
    // the next call takes as d_carry_in / d_carry_bits_in (nullptr: none).  max_frames >= frames_capacity(n_bits, period_bits).
    static size_t frames_capacity(size_t n_bits, size_t period_bits) { return vit_hip_frames_capacity(n_bits, period_bits); }
    void frames_extract(const uint8_t* d_bytes, size_t rows, size_t n_bits, size_t period_bits, size_t phase0,
                        const vit_hip_marker_lock* d_lock, const uint8_t* d_carry_in, const uint32_t* d_carry_bits_in, uint8_t* d_frames,
                        size_t max_frames, uint32_t* d_n_frames, uint8_t* d_carry_out, uint32_t* d_carry_bits_out,
                        uint32_t* d_marker_errors = nullptr, uint64_t marker = 0, unsigned marker_bits = 0, size_t drop_bits = 0,
                        const uint8_t* d_pad = nullptr, size_t bytes_row_stride = 0, size_t carry_row_stride = 0,
                        size_t frame_stride_bytes = 0, void* stream = nullptr) {
        check(vit_hip_frames_extract(m_hip, d_bytes, bytes_row_stride, rows, n_bits, period_bits, phase0, d_lock, d_carry_in,
                                     d_carry_bits_in, carry_row_stride, marker, marker_bits, drop_bits, d_pad, d_frames, frame_stride_bytes,
                                     max_frames, d_n_frames, d_marker_errors, d_carry_out, d_carry_bits_out, stream),
              "vit_hip_frames_extract");
    }
    // Reed-Solomon decoding (vit_hip_rs_create / vit_hip_rs_decode_batch): rs_create validates the code, builds its tables and uploads
    // them once; the caller frees it with rs_destroy before this decoder goes.  rs_decode decodes the interleaved codewords of the frames
    // frames_extract wrote -- frame (row, f) at d_in + (row * max_frames + f) * frame_stride_bytes (0: n * interleave), symbol i of codeword
    // c at byte i * interleave + c -- in place (d_out == d_in) or into a buffer of the same layout; d_n_frames [rows] (nullptr: all
    // max_frames) bounds the frames of a row that are touched; d_status [rows][max_frames][interleave] receives the byte errors corrected
    // or -1 for a codeword left as received.
    vit_hip_rs_code rs_create(const vit_hip_rs_params& params) {
        vit_hip_rs_code code = nullptr;
        check(vit_hip_rs_create(m_hip, &params, &code), "vit_hip_rs_create");
        return code;
    }
    static void rs_destroy(vit_hip_rs_code code) { vit_hip_rs_destroy(code); }
    void rs_decode(vit_hip_rs_code code, const uint8_t* d_in, uint8_t* d_out, size_t rows, size_t max_frames, const uint32_t* d_n_frames,
                   size_t interleave, int32_t* d_status, size_t frame_stride_bytes = 0, void* stream = nullptr) {
        check(vit_hip_rs_decode_batch(m_hip, code, d_in, d_out, frame_stride_bytes, rows, max_frames, d_n_frames, interleave, d_status, stream),
              "vit_hip_rs_decode_batch");
    }
    // The DVB-S stages on either side of rs_decode (vit_hip_deinterleave_batch / vit_hip_dvb_derandomize_batch).  deinterleave undoes the
    // convolutional interleaver (DVB-S: branches 12, cell 17, packet_bytes 204) on the packets frames_extract wrote: d_hist_in / d_fill_in
    // (nullptr: none) are the H = ceil((branches-1) * cell * branches / packet_bytes) packets the previous call left as d_hist_out /
    // d_fill_out, d_out / d_n_out [rows] receive the packets completed, compacted from packet 0 of every row, as rs_decode(interleave 1)
    // takes them.  dvb_derandomize XORs the energy-dispersal sequence off the first 188 bytes of every packet and puts the inverted
    // every-eighth sync byte upright; d_phase_in [rows] (nullptr or a value >= 8: voted from the sync bytes) is the place of packet 0 in its
    // group of eight, d_phase_out [rows] that of the next call's; d_rs_status [rows][max_frames] (may be nullptr) sets the
    // transport_error_indicator where negative, d_sync_errors [rows][max_frames] (may be nullptr) receives the sync byte's bit errors.
    void deinterleave(const uint8_t* d_in, size_t rows, size_t max_frames, const uint32_t* d_n_frames, size_t branches, size_t cell,
                      size_t packet_bytes, const uint8_t* d_hist_in, const uint32_t* d_fill_in, uint8_t* d_out, uint32_t* d_n_out,
                      uint8_t* d_hist_out, uint32_t* d_fill_out, size_t frame_stride_bytes = 0, size_t out_stride_bytes = 0,
                      size_t hist_row_stride = 0, void* stream = nullptr) {
        check(vit_hip_deinterleave_batch(m_hip, d_in, frame_stride_bytes, rows, max_frames, d_n_frames, branches, cell, packet_bytes, d_hist_in,
                                         d_fill_in, hist_row_stride, d_out, out_stride_bytes, d_n_out, d_hist_out, d_fill_out, stream),
              "vit_hip_deinterleave_batch");
    }
    void dvb_derandomize(const uint8_t* d_in, size_t packet_bytes, size_t rows, size_t max_frames, const uint32_t* d_n_frames,
                         const uint32_t* d_phase_in, uint8_t* d_out, uint32_t* d_phase_out, const int32_t* d_rs_status = nullptr,
                         uint32_t* d_sync_errors = nullptr, size_t frame_stride_bytes = 0, size_t out_stride_bytes = 0,
                         void* stream = nullptr) {
        check(vit_hip_dvb_derandomize_batch(m_hip, d_in, frame_stride_bytes, packet_bytes, rows, max_frames, d_n_frames, d_phase_in, d_rs_status,
                                            d_out, out_stride_bytes, d_phase_out, d_sync_errors, stream),
              "vit_hip_dvb_derandomize_batch");
    }
    // The frame check (vit_hip_crc_batch): the CRC `crc` = (width <= 32, poly, init, xorout), not reflected, of bits [first_bit, first_bit +
    // n_bits) of every frame in the layout above -- the frames rs_decode left, or with rows = 1 the bytes decode_tail_biting wrote.  d_crc
    // [rows][max_frames] (may be nullptr) receives the CRC, d_syndrome [rows][max_frames] (may be nullptr; one of the two is given) the CRC
    // XORed with the `width` bits behind the data: 0 where the frame checks, the RNTI on PDCCH.  d_n_frames [rows] (nullptr: all
    // max_frames) bounds the frames of a row that are touched.
    void crc_check(const vit_hip_crc_params& crc, const uint8_t* d_frames, size_t rows, size_t max_frames, const uint32_t* d_n_frames,
                   size_t first_bit, size_t n_bits, uint32_t* d_crc, uint32_t* d_syndrome, size_t frame_stride_bytes = 0,
                   void* stream = nullptr) {
        check(vit_hip_crc_batch(m_hip, &crc, d_frames, frame_stride_bytes, rows, max_frames, d_n_frames, first_bit, n_bits, d_crc, d_syndrome,
                                stream),
              "vit_hip_crc_batch");
    }
    // LTE rate de-matching (vit_hip_lte_rate_dematch_batch; 3GPP TS 36.212 5.1.4.2 undone) in front of decode_tail_biting: the soft bits
    // d_received [n_received] -> d_symbols_out [frames][D][3], a decoder of R = 3.  Frame f is the elements [base, base + E) with base =
    // d_offset ? d_offset[f] : f * received_frame_stride and E = min(d_count ? d_count[f] : E_max, E_max), cut at n_received; the
    // repetitions of a coded bit are added in int32, negated where the bit (base + k) mod scramble_period (0: base + k) of d_scramble
    // (MSB-first; nullptr: off) is set, rounded by (x + ((1 << shift) >> 1)) >> shift and clamped to [clamp_lo, clamp_hi]; 0 where
    // nothing was sent.
    void lte_rate_dematch(const soft_t* d_received, size_t n_received, size_t received_frame_stride, const uint32_t* d_offset,
                          const uint32_t* d_count, size_t frames, size_t D, size_t E_max, const uint8_t* d_scramble, size_t scramble_period,
                          unsigned shift, int clamp_lo, int clamp_hi, soft_t* d_symbols_out, void* stream = nullptr) {
        check(vit_hip_lte_rate_dematch_batch(m_hip, d_received, n_received, received_frame_stride, d_offset, d_count, frames, D, E_max,
                                             d_scramble, scramble_period, shift, clamp_lo, clamp_hi, d_symbols_out, stream),
              "vit_hip_lte_rate_dematch_batch");
    }
    // The DAB receive chain around decode (vit_hip_dab_deinterleave_batch / vit_hip_dab_descramble_batch; ETSI EN 300 401 clauses 12, 11
    // and 10).  dab_deinterleave undoes the time interleaver -- soft bit i of a frame was sent bitrev4(i mod 16) frames late -- on rows of
    // received frames of n_received soft bits (frame (r, f) at d_in + r * in_row_stride + f * in_frame_stride, 0: packed) and depunctures
    // through d_source_index [symbols_per_frame] (nullptr: the identity) in the same pass: d_out [rows][max_frames][symbols_per_frame]
    // receives the d_n_out[r] logical frames completed, 0 where the map names nothing.  d_hist_in / d_fill_in (nullptr: none) are the 15
    // frames the previous call left as d_hist_out / d_fill_out.  dab_descramble XORs the energy-dispersal sequence off the first n_bits
    // bits of every frame of decoded bytes (frame (r, f) at (r * max_frames + f) * stride, 0: ceil(n_bits / 8)); d_out == d_in is in place.
    void dab_deinterleave(const soft_t* d_in, size_t rows, size_t max_frames, const uint32_t* d_n_frames, size_t n_received,
                          const int32_t* d_source_index, size_t symbols_per_frame, const soft_t* d_hist_in, const uint32_t* d_fill_in,
                          soft_t* d_out, uint32_t* d_n_out, soft_t* d_hist_out, uint32_t* d_fill_out, size_t in_row_stride = 0,
                          size_t in_frame_stride = 0, size_t hist_row_stride = 0, void* stream = nullptr) {
        check(vit_hip_dab_deinterleave_batch(m_hip, d_in, in_row_stride, in_frame_stride, rows, max_frames, d_n_frames, n_received,
                                             d_source_index, symbols_per_frame, d_hist_in, d_fill_in, hist_row_stride, d_out, d_n_out,
                                             d_hist_out, d_fill_out, stream),
              "vit_hip_dab_deinterleave_batch");
    }
    void dab_descramble(const uint8_t* d_in, size_t rows, size_t max_frames, const uint32_t* d_n_frames, size_t n_bits, uint8_t* d_out,
                        size_t frame_stride_bytes = 0, size_t out_stride_bytes = 0, void* stream = nullptr) {
        check(vit_hip_dab_descramble_batch(m_hip, d_in, frame_stride_bytes, rows, max_frames, d_n_frames, n_bits, d_out, out_stride_bytes,
                                           stream),
              "vit_hip_dab_descramble_batch");
    }
    // DAB+ audio superframes (vit_hip_dabplus_sync / vit_hip_dabplus_au_batch; ETSI TS 102 563).  dabplus_sync counts, per phase
    // (frame0 + f) mod 5, the logical frames of frame_bytes = 24 s bytes whose first two bytes are the Fire code of the nine behind them,
    // into d_hits / d_count [rows][5] (flags as marker_search), and writes the lock frames_extract reads at period_bits = 40 * frame_bytes
    // into d_lock [rows] (may be nullptr).  dabplus_au_table reads the header of every superframe of 120 s bytes (rs_decode at interleave
    // s in front of it; d_rs_status may be nullptr) and writes d_info [rows * max_frames] and the six {start, bytes, syndrome} entries of
    // d_au: syndrome 0 where the access unit's CRC-16 checks.
    void dabplus_sync(const uint8_t* d_frames, size_t rows, size_t max_frames, const uint32_t* d_n_frames, size_t frame_bytes,
                      unsigned frame0, uint32_t* d_hits, uint32_t* d_count, vit_hip_marker_lock* d_lock = nullptr, unsigned flags = 0,
                      size_t row_stride = 0, size_t frame_stride = 0, void* stream = nullptr) {
        check(vit_hip_dabplus_sync(m_hip, d_frames, row_stride, frame_stride, frame_bytes, rows, max_frames, d_n_frames, frame0, flags,
                                   d_hits, d_count, d_lock, stream),
              "vit_hip_dabplus_sync");
    }
    void dabplus_au_table(const uint8_t* d_in, size_t rows, size_t max_frames, const uint32_t* d_n_frames, unsigned s,
                          const int32_t* d_rs_status, uint32_t* d_info, vit_hip_dabplus_au* d_au, size_t frame_stride_bytes = 0,
                          void* stream = nullptr) {
        check(vit_hip_dabplus_au_batch(m_hip, d_in, frame_stride_bytes, rows, max_frames, d_n_frames, s, d_rs_status, d_info, d_au, stream),
              "vit_hip_dabplus_au_batch");
    }
    // The IEEE 802.11a/g OFDM data path around decode (vit_hip_wifi_deinterleave_batch / _signal_batch / _data_batch), a decoder of K = 7,
    // R = 2 with the polynomials (109, 79).  wifi_deinterleave undoes the per-symbol interleaver and the puncturing of rate index 0 .. 7 in
    // one gather: frame f's max_sym * N_CBPS soft bits at d_in + f * in_frame_stride (0: max_sym * 288) -> d_symbols_out [frames][S][2], 0
    // behind the frame's n_steps.  d_rate / d_n_sym / d_n_steps (nullptr: `rate`, max_sym, n_sym * N_DBPS) are read at element f *
    // count_stride (0: 1): with 5 they point at the rate_index, n_sym and n_steps of the vit_hip_wifi_signal structs wifi_signal_parse
    // wrote from the 3 decoded bytes of every SIGNAL field.  wifi_descramble recovers the scrambler seed of the decoded DATA bytes,
    // descrambles, writes PSDU octets (frame f at d_psdu + f * psdu_stride, 0: max_length) and the FCS syndrome at the frame's own length.
    void wifi_deinterleave(const soft_t* d_in, size_t frames, size_t max_sym, size_t S, soft_t* d_symbols_out, unsigned rate = 0,
                           const uint32_t* d_rate = nullptr, const uint32_t* d_n_sym = nullptr, const uint32_t* d_n_steps = nullptr,
                           size_t count_stride = 0, size_t in_frame_stride = 0, void* stream = nullptr) {
        check(vit_hip_wifi_deinterleave_batch(m_hip, d_in, in_frame_stride, frames, max_sym, rate, d_rate, d_n_sym, d_n_steps, count_stride, S,
                                              d_symbols_out, stream),
              "vit_hip_wifi_deinterleave_batch");
    }
    void wifi_signal_parse(const uint8_t* d_bytes, size_t frames, vit_hip_wifi_signal* d_signal, size_t frame_stride_bytes = 0,
                           void* stream = nullptr) {
        check(vit_hip_wifi_signal_batch(m_hip, d_bytes, frame_stride_bytes, frames, d_signal, stream), "vit_hip_wifi_signal_batch");
    }
    void wifi_descramble(const uint8_t* d_bytes, size_t frames, size_t S, const uint32_t* d_length, size_t length_stride, size_t max_length,
                         uint8_t* d_psdu, vit_hip_wifi_status* d_status, size_t psdu_stride = 0, size_t frame_stride_bytes = 0,
                         void* stream = nullptr) {
        check(vit_hip_wifi_data_batch(m_hip, d_bytes, frame_stride_bytes, frames, S, d_length, length_stride, max_length, d_psdu, psdu_stride,
                                      d_status, stream),
              "vit_hip_wifi_data_batch");
    }
    // The front of the DVB-T route (vit_hip_dvbt_deinterleave_batch; ETSI EN 300 744 clauses 4.3.3 and 4.3.4), a decoder of K = 7, R = 2
    // with the polynomials (109, 79): the inner de-interleaver (symbol, bit, demultiplexer) fused with depuncturing.  Row r's n_sym OFDM
    // symbols [Nmax][v] at d_in + r * in_row_stride (0: n_sym * Nmax * v) -> n_sym * steps trellis steps (Y, X) at d_symbols_out + r *
    // out_row_stride * 2 (in steps; 0: n_sym * steps), 0 where the rate sent nothing: what decode_stream(s) reads.  mode 0 .. 2 = 2k, 4k,
    // 8k; v = 2, 4, 6; rate 0 .. 4 = 1/2, 2/3, 3/4, 5/6, 7/8.  The parity of a row's first symbol is `parity`, or d_parity_in[r]; with
    // d_parity_out the count goes on there (+ n_sym), ping-ponged between two arrays from call to call.
    void dvbt_deinterleave(const soft_t* d_in, size_t rows, size_t n_sym, unsigned mode, unsigned v, unsigned rate, soft_t* d_symbols_out,
                           unsigned parity = 0, const uint32_t* d_parity_in = nullptr, uint32_t* d_parity_out = nullptr,
                           size_t in_row_stride = 0, size_t out_row_stride = 0, void* stream = nullptr) {
        check(vit_hip_dvbt_deinterleave_batch(m_hip, d_in, in_row_stride, rows, n_sym, mode, v, rate, parity, d_parity_in, d_parity_out,
                                              d_symbols_out, out_row_stride, stream),
              "vit_hip_dvbt_deinterleave_batch");
    }
    // The IS-95A forward traffic channel, rate set 1 (vit_hip_is95_deinterleave_batch / vit_hip_is95_rate_decide_batch), a decoder of K = 9,
    // R = 2.  is95_deinterleave descrambles (d_scramble: 48 bytes a frame MSB-first at scramble_frame_stride bytes, 0: one mask for all;
    // nullptr: off), undoes the 384-symbol block interleaver and adds the repetitions under the four rate hypotheses in one launch:
    // d_out[h] (nullptr: not wanted; not all four) receives [frames][S_h][2], S_h = 192, 96, 48, 24, which decode reads with total_bits =
    // 184, 88, 40, 16; sums in int32, rounded by (x + ((1 << shift) >> 1)) >> shift, clamped to [clamp_lo, clamp_hi].  is95_rate_decide
    // picks, per frame, the hypothesis with the lowest errors / compared among those that are present (d_bytes[h] != nullptr), check
    // (d_syndrome[h] == 0, h < 2) and keep errors * ser_den <= compared * max_ser_num[h]: d_decision[f] = {rate (4: erased), info_bits,
    // errors, compared} and 22 info bytes at d_info + f * info_stride (0: 22), zero behind the winner's info bits.  The arrays of
    // pointers, strides and thresholds are host arrays of four (d_syndrome: two); bytes_frame_stride nullptr: 23, 11, 5, 2.
    void is95_deinterleave(const soft_t* d_in, size_t frames, soft_t* const d_out[4], const uint8_t* d_scramble = nullptr,
                           size_t scramble_frame_stride = 0, unsigned shift = 0, int clamp_lo = -127, int clamp_hi = 127,
                           size_t in_frame_stride = 0, void* stream = nullptr) {
        void* const out[4] = {d_out[0], d_out[1], d_out[2], d_out[3]};
        check(vit_hip_is95_deinterleave_batch(m_hip, d_in, in_frame_stride, frames, d_scramble, scramble_frame_stride, shift, clamp_lo,
                                              clamp_hi, out, stream),
              "vit_hip_is95_deinterleave_batch");
    }
    // the four re-encoded symbol error counts behind one zeroing kernel (vit_hip_is95_channel_errors_batch): what channel_errors writes for
    // every hypothesis with d_bytes[h] != nullptr, with no memset node in a captured graph
    void is95_channel_errors(const soft_t* const d_symbols[4], const uint8_t* const d_bytes[4], size_t frames, uint32_t* const d_errors[4],
                             uint32_t* const d_compared[4], const size_t* bytes_frame_stride = nullptr, void* stream = nullptr) {
        const void* const sym[4] = {d_symbols[0], d_symbols[1], d_symbols[2], d_symbols[3]};
        check(vit_hip_is95_channel_errors_batch(m_hip, sym, d_bytes, bytes_frame_stride, frames, d_errors, d_compared, stream),
              "vit_hip_is95_channel_errors_batch");
    }
    void is95_rate_decide(const uint8_t* const d_bytes[4], const uint32_t* const d_errors[4], const uint32_t* const d_compared[4],
                          const uint32_t* const d_syndrome[2], size_t frames, const uint32_t max_ser_num[4], uint32_t ser_den,
                          vit_hip_is95_decision* d_decision, uint8_t* d_info, size_t info_stride = 0,
                          const size_t* bytes_frame_stride = nullptr, void* stream = nullptr) {
        check(vit_hip_is95_rate_decide_batch(m_hip, d_bytes, bytes_frame_stride, d_errors, d_compared, d_syndrome, frames, max_ser_num,
                                             ser_den, d_decision, d_info, info_stride, stream),
              "vit_hip_is95_rate_decide_batch");
    }
    // GSM channel decoding (vit_hip_gsm_deinterleave_batch / vit_hip_gsm_fire_batch / vit_hip_gsm_tchfs_batch; 3GPP TS 45.003), a decoder of
    // K = 5, R = 2 with the polynomials (25, 27).  gsm_deinterleave reads `rows` rows of `bursts` = 4 m bursts of 116 soft_t (stealing flags
    // at 57 and 58) and undoes the block (mode VIT_HIP_GSM_BLOCK) or the diagonal (VIT_HIP_GSM_DIAGONAL: 8 bursts a block, four bursts of
    // history per row ping-ponged between d_hist_in / d_fill_in and d_hist_out / d_fill_out) interleaver: d_full [rows][m][228][2] is what
    // decode reads with total_bits = 224, d_class1 [rows][m][189][2] with 185, d_class2 [rows][m][78] the uncoded bits, d_steal [rows][m] the
    // sum of the stealing flags, d_n_out [rows] the blocks a row gave (m, or m - 1 without history); any output may be nullptr, not all
    // four.  gsm_fire checks the 40-bit Fire code of 28 decoded bytes a frame, corrects one error burst of at most max_burst <= 12 bits
    // and writes {status (0 clean, 1 .. 12 the burst corrected, -1 not correctable), first_bit, syndrome} and the 23 data bytes (in place
    // allowed; VIT_HIP_GSM_LSB_FIRST: octets LSB-first).  gsm_tchfs makes the 260-bit speech frame (33 bytes) of the 24 decoded class I
    // bytes and the 78 class II soft bits, with {parity_syndrome, class2_erasures}.
    void gsm_deinterleave(const soft_t* d_in, size_t rows, size_t bursts, unsigned mode, soft_t* d_full, soft_t* d_class1 = nullptr,
                          soft_t* d_class2 = nullptr, int32_t* d_steal = nullptr, uint32_t* d_n_out = nullptr, unsigned flags = 0,
                          const soft_t* d_hist_in = nullptr, const uint32_t* d_fill_in = nullptr, soft_t* d_hist_out = nullptr,
                          uint32_t* d_fill_out = nullptr, size_t in_row_stride = 0, size_t in_burst_stride = 0, void* stream = nullptr) {
        check(vit_hip_gsm_deinterleave_batch(m_hip, d_in, in_row_stride, in_burst_stride, rows, bursts, mode, flags, d_hist_in, d_fill_in,
                                             d_hist_out, d_fill_out, d_n_out, d_full, d_class1, d_class2, d_steal, stream),
              "vit_hip_gsm_deinterleave_batch");
    }
    void gsm_fire(const uint8_t* d_bytes, size_t frames, vit_hip_gsm_fire* d_status, uint8_t* d_data, unsigned max_burst = 12,
                  unsigned flags = 0, size_t bytes_frame_stride = 0, size_t data_stride = 0, void* stream = nullptr) {
        check(vit_hip_gsm_fire_batch(m_hip, d_bytes, bytes_frame_stride, frames, max_burst, flags, d_status, d_data, data_stride, stream),
              "vit_hip_gsm_fire_batch");
    }
    void gsm_tchfs(const uint8_t* d_bytes, const soft_t* d_class2, size_t frames, uint8_t* d_speech, vit_hip_gsm_tchfs* d_status = nullptr,
                   size_t bytes_frame_stride = 0, size_t speech_stride = 0, void* stream = nullptr) {
        check(vit_hip_gsm_tchfs_batch(m_hip, d_bytes, bytes_frame_stride, d_class2, frames, d_speech, speech_stride, d_status, stream),
              "vit_hip_gsm_tchfs_batch");
    }
    // multi-GPU set-up: the shared branch table and config travel once from rank `root` to every rank of an RCCL
    // communicator (ncclComm_t); each rank then constructs its own decoder from its copy.  The other ranks pass a table
    // built from any polynomials (it is overwritten) -- the reference shares one table between decoders (README.md:14)
    static void broadcast_table(void* nccl_comm, int root, int rank, BranchTable& table, Config& config, int device,
                                void* stream = nullptr) {
        check(vit_hip_broadcast_table(nccl_comm, root, rank, int(K), int(R), int(sizeof(soft_t)), int(sizeof(error_t)),
                                      table.data(), &config, device, stream), "vit_hip_broadcast_table");
        if (rank != root) table.refresh_levels();   // soft_decision_high()/low() must describe the rows that were received
    }
    vit_hip_handle hip_handle() const { return m_hip; }
    // which plan serves this code and whether a faster one exists (vit_hip_plan_note): one line of text
    const char* plan_note() const { return vit_hip_plan_note(m_hip); }

private:
    static size_t extension(size_t steps) { return steps ? steps : 8 * (K - 1); }
    static size_t window_or_default(size_t window) { return window ? window : 1024; }
    static unsigned stream_flags(bool begin, bool end) { return (begin ? VIT_HIP_STREAM_BEGIN : 0u) | (end ? VIT_HIP_STREAM_END : 0u); }
    static void check(int rc, const char* what) {
        if (rc != VIT_HIP_OK) {
            fprintf(stderr, "viterbi_hip: %s failed (%d): %s\n", what, rc, vit_hip_last_error());
            abort();
        }
    }
    vit_hip_handle m_hip = nullptr;
};

// Double-buffered pipeline over a batch decoder (vit_hip_pipeline_*): chainback of batch i runs beside the update of batch
// i+1 on a second stream.  submit() only enqueues; results of a batch are valid after a later sync().
template <size_t constraint_length, size_t code_rate, typename error_t, typename soft_t>
class ViterbiDecoder_HIP_Pipeline {
public:
    using Batch = ViterbiDecoder_HIP_Batch<constraint_length, code_rate, error_t, soft_t>;
    // `want`: schedule overrides (vit_hip_pipeline_options, struct_size set by the caller); nullptr: the library's rules
    ViterbiDecoder_HIP_Pipeline(Batch& decoder, size_t max_frames, size_t total_bits, const vit_hip_pipeline_options* want = nullptr) {
        if (vit_hip_pipeline_create_ex(decoder.hip_handle(), max_frames, total_bits, want, &m_pipe) != VIT_HIP_OK) die("vit_hip_pipeline_create_ex");
    }
    ~ViterbiDecoder_HIP_Pipeline() { vit_hip_pipeline_destroy(m_pipe); }
    ViterbiDecoder_HIP_Pipeline(const ViterbiDecoder_HIP_Pipeline&) = delete;
    ViterbiDecoder_HIP_Pipeline& operator=(const ViterbiDecoder_HIP_Pipeline&) = delete;
    void submit(const soft_t* d_symbols, size_t frames, uint8_t* d_bytes_out, const uint32_t* d_end_state = nullptr,
                void* done_event = nullptr) {
        if (vit_hip_pipeline_submit(m_pipe, d_symbols, frames, d_bytes_out, d_end_state, done_event) != VIT_HIP_OK) die("vit_hip_pipeline_submit");
    }
    void sync() {
        if (vit_hip_pipeline_sync(m_pipe) != VIT_HIP_OK) die("vit_hip_pipeline_sync");
    }
    // the pipeline runs on private non-blocking streams: order the NEXT submitted batch behind a hipEvent_t the producer of its
    // symbols recorded on its own stream (vit_hip_pipeline_wait_event); the other direction is submit()'s done_event
    void wait_event(void* producer_event) {
        if (vit_hip_pipeline_wait_event(m_pipe, producer_event) != VIT_HIP_OK) die("vit_hip_pipeline_wait_event");
    }
    // which schedule the library chose for max_frames: workspaces, update kernels in flight, chainback overlap
    vit_hip_pipeline_schedule schedule() const {
        vit_hip_pipeline_schedule s;
        if (vit_hip_pipeline_get_schedule_v2(m_pipe, &s, sizeof(s)) != VIT_HIP_OK) die("vit_hip_pipeline_get_schedule_v2");
        return s;
    }
    // per-batch kernel durations (HIP events on the kernels' own streams), the way the reference times update and chainback
    // separately (examples/run_benchmark.cpp:272-281); see vit_hip_pipeline_get_timing
    void set_timing(bool enable) {
        if (vit_hip_pipeline_set_timing(m_pipe, enable ? 1 : 0) != VIT_HIP_OK) die("vit_hip_pipeline_set_timing");
    }
    size_t timing(size_t capacity, float* update_ms, float* chainback_ms, float* complete_ms) const {
        size_t n = 0;
        if (vit_hip_pipeline_get_timing(m_pipe, capacity, update_ms, chainback_ms, complete_ms, &n) != VIT_HIP_OK) die("vit_hip_pipeline_get_timing");
        return n;
    }

private:
    static void die(const char* what) {
        fprintf(stderr, "viterbi_hip: %s failed: %s\n", what, vit_hip_last_error());
        abort();
    }
    vit_hip_pipeline_t m_pipe = nullptr;
};
