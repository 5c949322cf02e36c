// kernels_tb.hpp -- the side passes of tail-biting decoding (vit_hip_decode_tail_biting_batch), around the unchanged update and
// chainback kernels of every plan ("wrap-around Viterbi with fixed extension", DESIGN.md "Tail-biting frames"):
//   1. tb_gather_kernel     ext[f][e] = symbols[f][(e - head) mod L] for e in [0, head + L + tail), and every metric of every
//                           frame = initial_start_error (reset() with every state a start state), in one launch;
//   2. tb_select_*_kernel   per frame the state of smallest final metric (unsigned error_t, lowest index on a tie);
//   3. tb_window_kernel     decoded bytes = bits [head, head + L) of the chainback over the extension, and the flag that the
//                           path enters and leaves the window in the same state.
// All three are memory- or latency-bound and make one pass over their data.  They are not specialised on the polynomials: one
// instantiation per soft / error width.  Included only from vit_windows.hip (not from the register-plan units, whose kernel
// sources key the precompiled and run-time compiled caches).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vit {

struct TbGatherArgs {
    const void* symbols;     // [F][L][R] soft_t
    void* ext;               // [F][S_ext][R] soft_t, 256-byte aligned
    void* metrics;           // [F][N] error_t, 256-byte aligned
    uint64_t ext_elems;      // F * S_ext * R
    uint64_t gather_chunks;  // 16-byte chunks of ext: ceil(ext_elems * sizeof(soft_t) / 16)
    uint64_t metric_bytes;   // F * N * sizeof(error_t)
    uint64_t total_chunks;   // gather_chunks + ceil(metric_bytes / 16)
    uint32_t L, R, S_ext;
    uint32_t shift;          // (L - head % L) % L: ext step e reads symbol step (e + shift) mod L
    uint32_t fill;           // initial_start_error repeated over the four bytes of a dword (u16: twice, u8: four times)
};

// One thread per 16 bytes of output: the extension (16-byte stores, coalesced: a wavefront writes 1 KiB contiguous; the frame
// rows are not 16-byte multiples, so a chunk may straddle two frames), then the metrics behind it.  Grid-strided.
template <typename soft_t>
__global__ void __launch_bounds__(256) tb_gather_kernel(TbGatherArgs a) {
    constexpr uint32_t E = 16 / sizeof(soft_t);
    const uint64_t row = (uint64_t)a.S_ext * a.R;
    const soft_t* src = (const soft_t*)a.symbols;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.total_chunks; c += (uint64_t)gridDim.x * blockDim.x) {
        if (c < a.gather_chunks) {
            const uint64_t g0 = c * E;
            const uint64_t f = g0 / row;
            const uint32_t j = (uint32_t)(g0 - f * row);
            uint32_t e = j / a.R, r = j - e * a.R;
            uint32_t s = (uint32_t)(((uint64_t)e + a.shift) % a.L);
            // the source element walks forward one at a time: back by one frame row at the end of the frame's symbols, on to the next
            // frame's first extended step at the end of the extension
            const soft_t* p = src + (f * a.L + s) * a.R + r;
            const soft_t* frame = src + f * a.L * a.R;
            soft_t v[E];
#pragma unroll
            for (uint32_t k = 0; k < E; ++k) {
                v[k] = g0 + k < a.ext_elems ? *p : (soft_t)0;
                ++p;
                if (++r == a.R) {                                   // next trellis step
                    r = 0;
                    if (++s == a.L) {
                        s = 0;
                        p = frame;
                    }
                    if (++e == a.S_ext) {                           // next frame
                        e = 0;
                        s = a.shift;
                        frame += (size_t)a.L * a.R;
                        p = frame + (size_t)s * a.R;
                    }
                }
            }
            soft_t* dst = (soft_t*)a.ext + g0;
            if (g0 + E <= a.ext_elems) {
                uint4 w;
                __builtin_memcpy(&w, v, 16);
                *(uint4*)dst = w;
            } else {
                for (uint32_t k = 0; g0 + k < a.ext_elems; ++k) dst[k] = v[k];
            }
        } else {
            const uint64_t o = (c - a.gather_chunks) * 16;
            uint8_t* dst = (uint8_t*)a.metrics + o;
            if (o + 16 <= a.metric_bytes) {
                *(uint4*)dst = make_uint4(a.fill, a.fill, a.fill, a.fill);
            } else {
                for (uint64_t k = 0; o + k < a.metric_bytes; ++k) dst[k] = (uint8_t)(a.fill >> (8 * (k & 3)));
            }
        }
    }
}

struct TbSelectArgs {
    const void* metrics;     // [F][N] error_t
    uint32_t* end_ws;        // [F]: the end states chainback reads
    uint32_t* end_out;       // [F] or null: the caller's copy
    uint32_t frames, log2N;
    uint32_t keep_period;    // 0: every frame is written.  Else the frames f with f % keep_period == keep_phase keep the end state
    uint32_t keep_phase;     // the caller put there (vit_hip_decode_streams: the last window of every stream ends in state 0)
};

// such a frame's end state stays as it is
__device__ inline bool tb_select_keeps(const TbSelectArgs& a, uint32_t f) { return a.keep_period && f % a.keep_period == a.keep_phase; }

// the packed key (metric << log2 N) | state of VB / sizeof(error_t) consecutive states, reduced to the lane's minimum: the minimum
// key is the smallest metric (unsigned) and, among equal metrics, the lowest state.  log2 N <= 15 and error_t <= 16 bits: 31 bits.
template <typename error_t, int VB>
__device__ inline uint32_t tb_min_key(const uint8_t* p, uint32_t first_state, uint32_t log2N) {
    static_assert(VB == 16 || VB == 8 || VB == 4 || VB == 2, "one 16-, 8-, 4- or 2-byte load");
    static_assert(VB >= (int)sizeof(error_t), "at least one state per lane");
    uint32_t w[VB >= 4 ? VB / 4 : 1];
    if constexpr (VB == 16) {
        const uint4 x = *(const uint4*)p;
        w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
    } else if constexpr (VB == 8) {
        const uint2 x = *(const uint2*)p;
        w[0] = x.x; w[1] = x.y;
    } else if constexpr (VB == 4) {
        w[0] = *(const uint32_t*)p;
    } else {
        w[0] = *(const uint16_t*)p;                      // K = 2 with 8-bit metrics: the frame's whole 2 bytes
    }
    constexpr int V = VB / (int)sizeof(error_t);
    uint32_t best = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const uint32_t m = sizeof(error_t) == 2 ? (w[k / 2] >> (16 * (k & 1))) & 0xFFFFu : (w[k / 4] >> (8 * (k & 3))) & 0xFFu;
        const uint32_t key = (m << log2N) | (first_state + (uint32_t)k);
        best = key < best ? key : best;
    }
    return best;
}

// K <= 9 (N <= 256): P = N * sizeof(error_t) / VB lanes per frame (1 <= P <= 32), each with VB contiguous bytes of metrics (one
// 16-, 8-, 4- or 2-byte load, never past its frame: VB = min(16, N * sizeof(error_t))); a wavefront serves 64 / P frames and
// reduces each group of P lanes with xor shuffles (the groups are aligned).
template <typename error_t, int VB>
__global__ void __launch_bounds__(256) tb_select_small_kernel(TbSelectArgs a) {
    const uint32_t N = 1u << a.log2N;
    const uint32_t P = N * (uint32_t)sizeof(error_t) / VB;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t f = (uint32_t)(t / P), p = (uint32_t)(t % P);
    uint32_t key = 0xFFFFFFFFu;
    if (f < a.frames)
        key = tb_min_key<error_t, VB>((const uint8_t*)a.metrics + ((size_t)f * N * sizeof(error_t) + (size_t)p * VB),
                                      p * (VB / (uint32_t)sizeof(error_t)), a.log2N);
    for (uint32_t off = P / 2; off >= 1; off >>= 1) {
        const uint32_t o = __shfl_xor(key, (int)off);
        key = o < key ? o : key;
    }
    if (f < a.frames && p == 0 && !tb_select_keeps(a, f)) {
        const uint32_t s = key & (N - 1u);
        a.end_ws[f] = s;
        if (a.end_out) a.end_out[f] = s;
    }
}

// K >= 10 (N up to 32768): one workgroup of 256 per frame, 16-byte loads strided over the frame's metrics, a wavefront reduction,
// then the four wavefront minima through LDS.
template <typename error_t>
__global__ void __launch_bounds__(256) tb_select_large_kernel(TbSelectArgs a) {
    __shared__ uint32_t part[4];
    const uint32_t N = 1u << a.log2N;
    const uint32_t f = blockIdx.x;
    constexpr uint32_t V = 16 / sizeof(error_t);
    const uint32_t chunks = N / V;
    const uint8_t* base = (const uint8_t*)a.metrics + (size_t)f * N * sizeof(error_t);
    uint32_t key = 0xFFFFFFFFu;
    for (uint32_t c = threadIdx.x; c < chunks; c += blockDim.x) {
        const uint32_t k = tb_min_key<error_t, 16>(base + (size_t)c * 16, c * V, a.log2N);
        key = k < key ? k : key;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t o = __shfl_xor(key, off);
        key = o < key ? o : key;
    }
    if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = key;
    __syncthreads();
    if (threadIdx.x == 0 && !tb_select_keeps(a, f)) {
        for (uint32_t w = 1; w < blockDim.x / 64; ++w) key = part[w] < key ? part[w] : key;
        const uint32_t s = key & (N - 1u);
        a.end_ws[f] = s;
        if (a.end_out) a.end_out[f] = s;
    }
}

struct TbWindowArgs {
    const uint8_t* ext_bytes;  // [F][nbe]: chainback over the extension, MSB-first
    uint8_t* out;              // [F][nb], nb = ceil(L / 8)
    uint8_t* ok;               // [F] or null
    uint64_t total;            // F * nb
    uint32_t nbe, nb, L, head, K;
};

// n <= 15 bits of a frame's extended chainback starting at bit `pos` (MSB-first), as an integer whose last bit is bit pos + n - 1
__device__ inline uint32_t tb_bits(const uint8_t* row, uint32_t pos, uint32_t n) {
    const uint32_t b0 = pos >> 3, b1 = (pos + n - 1) >> 3;
    uint32_t v = 0;
    for (uint32_t b = b0; b <= b1; ++b) v = (v << 8) | row[b];
    return (v >> (8 * (b1 - b0 + 1) - (pos & 7) - n)) & ((1u << n) - 1u);
}

// one thread per output byte: the two extended bytes that straddle bit head + 8 i, shifted by head % 8, pad bits past L cleared
__global__ void __launch_bounds__(256) tb_window_kernel(TbWindowArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const uint32_t f = (uint32_t)(i / a.nb), b = (uint32_t)(i - (uint64_t)f * a.nb);
    const uint8_t* row = a.ext_bytes + (size_t)f * a.nbe;
    const uint32_t j = (a.head >> 3) + b, sh = a.head & 7u;
    uint32_t v = (uint32_t)row[j] << 8;
    if (sh && j + 1 < a.nbe) v |= row[j + 1];
    uint32_t byte = (v >> (8 - sh)) & 0xFFu;
    const uint32_t rem = a.L - 8 * b;                 // bits of the frame from this byte on
    if (rem < 8) byte &= 0xFFu << (8 - rem);
    a.out[i] = (uint8_t)byte;
    if (a.ok && b == 0) {
        const uint32_t n = a.K - 1;
        a.ok[f] = tb_bits(row, a.head - n, n) == tb_bits(row, a.head + a.L - n, n) ? 1 : 0;
    }
}

// ---- launchers (hipGetLastError() after each: 0 / -1) -----------------------------------------------------------------------

// workgroups of 256 for `threads` threads, at least one and at most `cap` (kernels_stream.hpp uses it too)
inline unsigned tb_blocks(uint64_t threads, uint64_t cap) {
    const uint64_t b = (threads + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

inline int tb_launch_gather(int soft_bytes, const TbGatherArgs& a, hipStream_t st) {
    const unsigned blocks = tb_blocks(a.total_chunks, 8192);          // memory-bound: grid-stride past 8192 blocks
    if (soft_bytes == 2) hipLaunchKernelGGL(tb_gather_kernel<int16_t>, dim3(blocks), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(tb_gather_kernel<int8_t>, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int tb_launch_select(int error_bytes, const TbSelectArgs& a, hipStream_t st) {
    // a shape no kernel below serves is refused, never launched
    if ((error_bytes != 1 && error_bytes != 2) || a.log2N < 1 || a.log2N > 15) return -1;
    const uint32_t N = 1u << a.log2N;
    if (a.log2N >= 9) {
        if (error_bytes == 2) hipLaunchKernelGGL(tb_select_large_kernel<uint16_t>, dim3(a.frames), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(tb_select_large_kernel<uint8_t>, dim3(a.frames), dim3(256), 0, st, a);
        return hipGetLastError() == hipSuccess ? 0 : -1;
    }
    const uint32_t bytes = N * (uint32_t)error_bytes;                // 2 .. 512 per frame
    const uint32_t vb = bytes >= 16 ? 16 : bytes;                     // 16, 8, 4 or 2: P = bytes / vb >= 1 lanes per frame
    const uint64_t lanes = (uint64_t)a.frames * (bytes / vb);
    const unsigned blocks = tb_blocks(lanes, 0xFFFFFFFFull);
    if (error_bytes == 2) {
        if (vb == 16) hipLaunchKernelGGL((tb_select_small_kernel<uint16_t, 16>), dim3(blocks), dim3(256), 0, st, a);
        else if (vb == 8) hipLaunchKernelGGL((tb_select_small_kernel<uint16_t, 8>), dim3(blocks), dim3(256), 0, st, a);
        else if (vb == 4) hipLaunchKernelGGL((tb_select_small_kernel<uint16_t, 4>), dim3(blocks), dim3(256), 0, st, a);
        else return -1;
    } else {
        if (vb == 16) hipLaunchKernelGGL((tb_select_small_kernel<uint8_t, 16>), dim3(blocks), dim3(256), 0, st, a);
        else if (vb == 8) hipLaunchKernelGGL((tb_select_small_kernel<uint8_t, 8>), dim3(blocks), dim3(256), 0, st, a);
        else if (vb == 4) hipLaunchKernelGGL((tb_select_small_kernel<uint8_t, 4>), dim3(blocks), dim3(256), 0, st, a);
        else if (vb == 2) hipLaunchKernelGGL((tb_select_small_kernel<uint8_t, 2>), dim3(blocks), dim3(256), 0, st, a);
        else return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

inline int tb_launch_window(const TbWindowArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(tb_window_kernel, dim3(tb_blocks(a.total, 0xFFFFFFFFull)), dim3(256), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace vit
