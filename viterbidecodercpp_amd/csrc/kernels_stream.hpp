// kernels_stream.hpp -- the side passes of overlapped-window decoding of long streams (vit_hip_decode_stream: one stream;
// vit_hip_decode_streams: several in lockstep on one window grid), around the unchanged update, end-state select (kernels_tb.hpp)
// and chainback kernels of every plan (DESIGN.md "One long stream", "Many streams on one window grid"):
//   1. stream_init_kernel    the start metrics of every window: initial_start_error in every state (the tail-biting start), the
//                            reset(0) pattern for window 0 of every stream under BEGIN, and end state 0 for the last window of
//                            every stream under END;
//   2. stream_stitch_kernel  per stream the one contiguous output bit stream from the windows' chainback rows: window i
//                            contributes bits [head, head + W) of its row (window 0 under BEGIN from bit 0, the last window up to
//                            the end of the emitted range).
// With several streams the uniform windows of all of them are rows of ONE grid: stream s's window i is row s * period + i, and the
// rows between one stream's last window and the next one's first (the bridge windows, which straddle two segments) are initialised
// like any other and never read by the stitch.  One stream is the case n_streams = 1.
// Both are memory-bound and make one pass over their data; neither is specialised on the polynomials.  Included only from
// vit_windows.hip (not from the register-plan units, whose kernel sources key the precompiled and run-time compiled caches).
#pragma once
#include "kernels_tb.hpp"

namespace vit {

struct StreamInitArgs {
    void* met_u;             // [rows_u][N] error_t: the grid windows' metrics, 256-byte aligned
    void* met_r;             // [n_streams][N] error_t: the remainder windows' metrics, 256-byte aligned (unused when bytes_r == 0)
    uint32_t* end_zero;      // under END the end state of every stream's last window, forced to 0: end_zero[z * end_zero_stride]
    uint32_t end_zero_count; //   for z < end_zero_count (n_streams, or 0 without END)
    uint32_t end_zero_stride;
    uint64_t bytes_u;        // rows_u * N * sizeof(error_t)
    uint64_t bytes_r;        // n_streams * N * sizeof(error_t) or 0
    uint64_t chunks_u;       // ceil(bytes_u / 16)
    uint64_t total_chunks;   // chunks_u + ceil(bytes_r / 16)
    uint32_t row_bytes;      // N * sizeof(error_t): a power of two
    uint32_t row_shift;      // its log2
    uint32_t fill;           // initial_start_error repeated over the four bytes of a dword
    uint32_t non_start;      // initial_non_start_error, the same way
    uint32_t begin_period_u; // BEGIN: the rows of met_u that are a stream's window 0 (row % begin_period_u == 0) start from reset(0);
                             //   0: none does
    uint32_t begin_r;        // 1: so does every row of met_r (BEGIN and each stream is one remainder window)
};

// One thread per 16 bytes of metrics, grid-strided.  Only the chunks of a window-0 row differ under BEGIN: state 0 keeps
// initial_start_error, every other state gets initial_non_start_error.  A row may be shorter than a chunk (K <= 4).
template <typename error_t>
__global__ void __launch_bounds__(256) stream_init_kernel(StreamInitArgs a) {
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t z = t0; z < a.end_zero_count; z += step) a.end_zero[z * a.end_zero_stride] = 0u;
    for (uint64_t c = t0; c < a.total_chunks; c += step) {
        const bool in_u = c < a.chunks_u;
        const uint64_t o = (in_u ? c : c - a.chunks_u) * 16;
        const uint64_t bytes = in_u ? a.bytes_u : a.bytes_r;
        uint8_t* dst = (uint8_t*)(in_u ? a.met_u : a.met_r) + o;
        uint32_t w[4] = {a.fill, a.fill, a.fill, a.fill};
        const uint32_t period = in_u ? a.begin_period_u : a.begin_r;
        if (period) {
            const uint64_t last = o + 16 <= bytes ? o + 15 : bytes - 1;
            const uint32_t r0 = (uint32_t)(o >> a.row_shift), r1 = (uint32_t)(last >> a.row_shift);   // rows < 2^31
            if (r0 != r1 || r0 % period == 0) {
#pragma unroll
                for (uint32_t k = 0; k < 16; ++k) {
                    const uint64_t p = o + k;
                    const uint32_t row = (uint32_t)(p >> a.row_shift), in_row = (uint32_t)p & (a.row_bytes - 1u);
                    if (p < bytes && in_row >= (uint32_t)sizeof(error_t) && row % period == 0) {   // not state 0, in a window-0 row
                        const uint32_t sh = 8 * (k & 3);
                        w[k >> 2] = (w[k >> 2] & ~(0xFFu << sh)) | (a.non_start & (0xFFu << sh));
                    }
                }
            }
        }
        if (o + 16 <= bytes) {
            *(uint4*)dst = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (uint64_t k = 0; o + k < bytes; ++k) dst[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
    }
}

struct StreamStitchArgs {
    const uint8_t* rows_u;   // [rows_u][nbe_u]: the grid windows' chainback bytes, MSB-first; stream s's window i is row s * period + i
    const uint8_t* row_r;    // [n_streams][nbe_r]: the remainder windows' (window n - 1 of every stream when n_u < n)
    uint8_t* out;            // [n_streams][out_pitch], of which [nb] are written: bits [a, b) of the segment, MSB-first, pad bits 0
    uint64_t out_pitch;      // bytes between the rows of out
    uint32_t n_streams;
    uint32_t period;         // grid windows from one stream's window 0 to the next one's (pitch / W)
    uint64_t nb;             // ceil((b - a) / 8)
    uint64_t chunks;         // ceil(nb / 16)
    uint32_t a, b;           // the emitted range, in steps of the segment
    uint32_t n, n_u;         // windows; of which in rows_u (n_u == n or n - 1)
    uint32_t W, head;
    uint32_t nbe_u, nbe_r;
    uint32_t out_aligned;    // every row of out is 16-byte aligned
};

// 8 bits of a row from bit q on (MSB-first); bits past the row's last byte read 0
__device__ inline uint32_t stream_bits8(const uint8_t* row, uint32_t nbe, uint32_t q) {
    const uint32_t j = q >> 3, sh = q & 7u;
    uint32_t v = (uint32_t)row[j] << 8;
    if (sh && j + 1 < nbe) v |= row[j + 1];
    return (v >> (8 - sh)) & 0xFFu;
}

__device__ inline uint32_t stream_load_u32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);               // the rows are byte-addressed: an unaligned dword load
    return v;
}

// One thread per 16 bytes of output.  A piece that lies inside one window (all but one in W / 128 of them) is five loads of the
// window's row -- four dwords and the byte behind them -- funnel-shifted by the row position's sub-byte part; a piece that crosses a
// window boundary (W and head need not be multiples of 8, and W may be as small as 8) is built byte by byte, each byte from the one
// or two windows it spans: a byte never spans three, as W >= 8.  The store is one 16-byte store per thread, coalesced.
// `a` arrives with rows_u, row_r and out at the stream's own rows.
__device__ inline void stream_stitch_piece(const StreamStitchArgs& a, uint64_t c) {
    const uint64_t byte0 = c * 16;
    const uint32_t p0 = a.a + (uint32_t)(byte0 * 8);                 // first step of the piece: < b <= T < 2^31
    // the window that emits step p: 0 below head (BEGIN only), else (p - head) / W capped at the last window
    uint32_t i = p0 < a.head ? 0u : (p0 - a.head) / a.W;
    if (i > a.n - 1) i = a.n - 1;
    // e: end of window i's share of the output
    uint32_t e = i == a.n - 1 ? a.b : a.head + (i + 1) * a.W;
    const uint8_t* row = i < a.n_u ? a.rows_u + (size_t)i * a.nbe_u : a.row_r;
    uint32_t nbe = i < a.n_u ? a.nbe_u : a.nbe_r;
    uint32_t w[4];
    const bool full = byte0 + 16 <= a.nb && (uint64_t)p0 + 128 <= a.b;
    if (full && (uint64_t)p0 + 128 <= e) {
        const uint32_t q = p0 - i * a.W;                             // position in the window's row
        const uint8_t* s = row + (q >> 3);
        const uint32_t sh = q & 7u;
        uint32_t B[5];
#pragma unroll
        for (int k = 0; k < 4; ++k) B[k] = __builtin_bswap32(stream_load_u32(s + 4 * k));
        B[4] = sh ? (uint32_t)s[16] << 24 : 0u;                      // bit q + 127 lies in byte 16 exactly when sh != 0
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = __builtin_bswap32(__funnelshift_l(B[k + 1], B[k], sh));
    } else {
        w[0] = w[1] = w[2] = w[3] = 0u;
        uint32_t p = p0;
        for (uint32_t k = 0; k < 16 && byte0 + k < a.nb; ++k, p += 8) {
            while (p >= e) {                                         // p < b: there is a next window
                ++i;
                e = i == a.n - 1 ? a.b : a.head + (i + 1) * a.W;
                row = i < a.n_u ? a.rows_u + (size_t)i * a.nbe_u : a.row_r;
                nbe = i < a.n_u ? a.nbe_u : a.nbe_r;
            }
            uint32_t byte = stream_bits8(row, nbe, p - i * a.W);
            const uint32_t m = e - p;                                // bits of this byte window i emits
            if (m < 8 && e < a.b) {                                  // the rest from the next window, whose share starts at its bit head
                const uint32_t j = i + 1;
                const uint8_t* row1 = j < a.n_u ? a.rows_u + (size_t)j * a.nbe_u : a.row_r;
                byte = (byte & (0xFFu << (8 - m))) | (stream_bits8(row1, j < a.n_u ? a.nbe_u : a.nbe_r, a.head) >> m);
            }
            const uint32_t rem = a.b - p;                            // bits of the output from this byte on
            if (rem < 8) byte &= 0xFFu << (8 - rem);
            w[k >> 2] |= byte << (8 * (k & 3));
        }
    }
    uint8_t* dst = a.out + byte0;
    if (a.out_aligned && byte0 + 16 <= a.nb) {
        *(uint4*)dst = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (uint32_t k = 0; k < 16 && byte0 + k < a.nb; ++k) dst[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

// blockIdx.x: 256 pieces of a row; blockIdx.y: the stream, strided when there are more streams than the grid's y extent
__global__ void __launch_bounds__(256) stream_stitch_kernel(StreamStitchArgs a) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.chunks) return;
    const uint8_t* rows_u = a.rows_u;
    const uint8_t* row_r = a.row_r;
    uint8_t* out = a.out;
    for (uint32_t s = blockIdx.y; s < a.n_streams; s += gridDim.y) {
        a.rows_u = rows_u + (size_t)s * a.period * a.nbe_u;
        a.row_r = row_r + (size_t)s * a.nbe_r;
        a.out = out + (size_t)s * a.out_pitch;
        stream_stitch_piece(a, c);
    }
}

// ---- launchers (hipGetLastError() after each: 0 / -1) -----------------------------------------------------------------------

inline int stream_launch_init(int error_bytes, const StreamInitArgs& a, hipStream_t st) {
    const unsigned blocks = tb_blocks(a.total_chunks, 8192);          // memory-bound: grid-stride past 8192 blocks
    if (error_bytes == 2) hipLaunchKernelGGL(stream_init_kernel<uint16_t>, dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(stream_init_kernel<uint8_t>, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int stream_launch_stitch(const StreamStitchArgs& a, hipStream_t st) {
    const unsigned ny = a.n_streams < 65535u ? a.n_streams : 65535u;
    hipLaunchKernelGGL(stream_stitch_kernel, dim3(tb_blocks(a.chunks, 0xFFFFFFFFull), ny), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
