// kvq_fp8.hip -- per-tensor fp8 (OCP e4m3fn) quantisation for the fp8 forward GEMMs of BASELINE.json configs[4] (gfx950).
//
// Extension: the reference is f32 throughout; off unless the engine is built with fp8 forward GEMMs.
//   y = x . W^T + b  (modeling_bert.py:139-352 behind models/bagon/Bagon.py:46-53)  becomes
//   y = (sat(x * sx) . sat(W * sw)^T) / (sx * sw) + b   with sx = 448 / amax|x|, sw = 448 / amax|W| (448 = largest e4m3 value),
// Weights: scales from the tensor that is quantised, in the same step (the whole flat bf16 shadow buffer in two launches per
// optimiser step, one scale per GEMM weight; a segment table maps buffer ranges to weights).  Activations, as the engine uses
// them: DELAYED scaling (kvq_fp8_quantize_delayed): one pass that quantises with the scale derived from the previous call's
// amax at that site (4x headroom, kvq_fp8_update_scales) and records this call's amax; the first call at a site runs with
// scale 1 and saturates at +-448.  kvq_fp8_quantize (amax pass + quantise pass, scale of the same tensor) is the two-launch
// form without history.  A NaN stays a NaN through the quantisation (the clamp lets it pass), so a diverged activation shows.
// Input-gradient GEMMs on fp8 (option): the same passes with the format as an argument (kvq_fp8_*_fmt: gradients
// go to OCP e5m2, largest value 57344) and the byte transpose of the e4m3 weight mirror (kvq_fp8_transpose[_segments]).
#include "kvq_common.h"

namespace kvq {

constexpr int Q_THREADS = 256;
// (FP8_MAX, amax8, quant8, fp8_amax_note: kvq_common.h -- the producers of csrc/kvq_ln.hip / kvq_nn.hip / kvq_gemm2.hip emit the same bytes)

__device__ __forceinline__ void block_amax_to(float m, float* dst) {
    __shared__ float sm[Q_THREADS / WAVE];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = sm[0];
#pragma unroll
        for (int i = 1; i < Q_THREADS / WAVE; ++i) t = fmaxf(t, sm[i]);
        atomicMax(reinterpret_cast<unsigned*>(dst), __float_as_uint(t));          // non-negative floats order like their bit patterns
    }
}

__device__ __forceinline__ float scale_of(float amax) { return amax > 0.f ? FP8_MAX / amax : 1.0f; }

// amax accumulators are zeroed by a KERNEL, not hipMemsetAsync: a memset captured into a hipGraph is a node of another kind and
// was the one thing in the replayed fp8 step that did not keep its place in the stream's order -- with 123 segments two identically
// seeded runs parted ways after 8 - 14 steps (an amax cleared after the first maxima had landed), eager launches never did
// (tools/fp8_flake.py, profiles/r04_fp8.md)
// `step` / `period` (weights inside the training step, kvq_fp8_quantize_segments_periodic): the amax accumulators are refreshed only
// on steps that are multiples of `period` -- the step count is read on the DEVICE, so a replayed graph takes the same decision as
// an eager step
__global__ __launch_bounds__(256) void fp8_zero_kernel(float* __restrict__ p, int n, const unsigned long long* __restrict__ step = nullptr,
                                                       int period = 1) {
    if (step && period > 1 && (*step % (unsigned long long)period) != 0) return;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) p[i] = 0.f;
}

// segments: seg s covers elements [off[s], off[s] + n[s]) of src (bf16) / dst (fp8), n[s] % 8 == 0, off[s] % 8 == 0
__global__ __launch_bounds__(Q_THREADS) void fp8_seg_amax_kernel(const unsigned short* __restrict__ src, const int64_t* __restrict__ off,
                                                                  const int64_t* __restrict__ n, float* __restrict__ amax,
                                                                  const unsigned long long* __restrict__ step = nullptr, int period = 1) {
    if (step && period > 1 && (*step % (unsigned long long)period) != 0) return;      // (uniform over the grid)
    const int s = blockIdx.y;
    const int64_t chunks = n[s] >> 3;
    const uint4* p = reinterpret_cast<const uint4*>(src + off[s]);
    float m = 0.f;
    for (int64_t c = (int64_t)blockIdx.x * Q_THREADS + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * Q_THREADS) m = fmaxf(m, amax8(p[c]));
    block_amax_to(m, amax + s);
}

__global__ __launch_bounds__(Q_THREADS) void fp8_seg_quant_kernel(const unsigned short* __restrict__ src, const int64_t* __restrict__ off,
                                                                   const int64_t* __restrict__ n, const float* __restrict__ amax,
                                                                   unsigned char* __restrict__ dst, float* __restrict__ scale,
                                                                   const unsigned long long* __restrict__ step = nullptr, int period = 1) {
    // (period < 0: the conversion is gated like the amax pass -- the Adam kernel wrote this step's bytes with the scales in force)
    if (step && period < -1 && (*step % (unsigned long long)(-period)) != 0) return;
    const int s = blockIdx.y;
    const int64_t chunks = n[s] >> 3;
    const float sc = scale_of(amax[s]);
    const uint4* p = reinterpret_cast<const uint4*>(src + off[s]);
    uint2* q = reinterpret_cast<uint2*>(dst + off[s]);
    for (int64_t c = (int64_t)blockIdx.x * Q_THREADS + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * Q_THREADS) q[c] = quant8(p[c], sc);
    if (blockIdx.x == 0 && threadIdx.x == 0) scale[s] = sc;
}

// one tensor, rows of `cols` elements with row stride ld (elements): activations
__global__ __launch_bounds__(Q_THREADS) void fp8_amax_kernel(const unsigned short* __restrict__ src, int64_t rows, int cols, int64_t ld,
                                                              float* __restrict__ amax) {
    const int cpr = cols >> 3;
    const int64_t chunks = rows * cpr;
    float m = 0.f;
    for (int64_t c = (int64_t)blockIdx.x * Q_THREADS + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * Q_THREADS) {
        const int64_t r = c / cpr;
        m = fmaxf(m, amax8(*reinterpret_cast<const uint4*>(src + r * ld + (c - r * cpr) * 8)));
    }
    block_amax_to(m, amax);
}

__global__ __launch_bounds__(Q_THREADS) void fp8_quant_kernel(const unsigned short* __restrict__ src, int64_t rows, int cols, int64_t ld,
                                                               const float* __restrict__ amax, unsigned char* __restrict__ dst,
                                                               float* __restrict__ scale) {
    const int cpr = cols >> 3;
    const int64_t chunks = rows * cpr;
    const float sc = scale_of(amax[0]);
    for (int64_t c = (int64_t)blockIdx.x * Q_THREADS + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * Q_THREADS) {
        const int64_t r = c / cpr;
        *reinterpret_cast<uint2*>(dst + c * 8) = quant8(*reinterpret_cast<const uint4*>(src + r * ld + (c - r * cpr) * 8), sc);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) scale[0] = sc;
}

// Delayed scaling for activations: quantise with the scale derived from the PREVIOUS call's amax at this site and record this
// call's amax on the way -- one pass over the tensor instead of two.  A value beyond the previous range saturates;
// kvq_fp8_update_scales leaves `headroom` (4x) between the last amax and 448, which costs an fp format no precision, only
// underflow range.  state (per site) = {scale, unused x 7, partial amax of each of the Q_PARTS workgroups}: plain stores, no
// atomics (a thousand atomicMax on one word serialise at ~12 ns each: measured 28 us per call for a 4-us copy).
constexpr int Q_PARTS = 512;                    // workgroups of the quantisation pass: it writes slots 0 .. 511
constexpr int Q_STATE = 8 + FP8_PARTS;          // floats per site (the producers of round 5 spread their atomic maxima over 4096 slots)

__global__ __launch_bounds__(Q_THREADS) void fp8_quant_delayed_kernel(const unsigned short* __restrict__ src, int64_t rows, int cols, int64_t ld,
                                                                       unsigned char* __restrict__ dst, float* __restrict__ state) {
    __shared__ float sm[Q_THREADS / WAVE];
    const int cpr = cols >> 3;
    const int64_t chunks = rows * cpr;
    const float sc = state[0];
    float m = 0.f;
    if (ld == cols) {                                                       // dense: no row arithmetic
        const uint4* p = reinterpret_cast<const uint4*>(src);
        uint2* q = reinterpret_cast<uint2*>(dst);
        for (int64_t c = (int64_t)blockIdx.x * Q_THREADS + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * Q_THREADS) {
            const uint4 v = p[c];
            m = fmaxf(m, amax8(v));
            q[c] = quant8(v, sc);
        }
    } else {
        for (int64_t c = (int64_t)blockIdx.x * Q_THREADS + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * Q_THREADS) {
            const int64_t r = c / cpr;
            const uint4 v = *reinterpret_cast<const uint4*>(src + r * ld + (c - r * cpr) * 8);
            m = fmaxf(m, amax8(v));
            *reinterpret_cast<uint2*>(dst + c * 8) = quant8(v, sc);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = sm[0];
#pragma unroll
        for (int i = 1; i < Q_THREADS / WAVE; ++i) t = fmaxf(t, sm[i]);
        state[8 + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(Q_THREADS) void fp8_update_scales_kernel(float* state, float headroom) {
    __shared__ float sm[Q_THREADS / WAVE];
    float* st = state + (size_t)blockIdx.x * Q_STATE;
    float m = 0.f;
    for (int i = threadIdx.x; i < FP8_PARTS; i += Q_THREADS) {
        m = fmaxf(m, st[8 + i]);
        st[8 + i] = 0.f;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = sm[0];
#pragma unroll
        for (int i = 1; i < Q_THREADS / WAVE; ++i) t = fmaxf(t, sm[i]);
        if (t > 0.f && headroom > 0.f) st[0] = FP8_MAX / (t * headroom);  // a site that was not visited keeps its scale; headroom 0: only clear
    }
}

// ---- the same passes with the target format as a template argument (kvq_fp8_*_fmt): e5m2 for the gradients of the fp8
//      input-gradient GEMMs.  WIDE (cols % 16 == 0): a thread converts 16 elements -- two 16-byte loads, ONE 16-byte store (8-byte
//      accesses run at 0.54 - 0.70x the 16-byte rate, kvq_common.h).  dst == nullptr: only the amax is noted (the calibration step).
template <int FMT>
__global__ __launch_bounds__(Q_THREADS) void fp8_quant_fmt_kernel(const unsigned short* __restrict__ src, int64_t rows, int cols, int64_t ld,
                                                                   const float* __restrict__ amax, unsigned char* __restrict__ dst,
                                                                   float* __restrict__ scale) {
    const int cpr = cols >> 3;
    const int64_t chunks = rows * cpr;
    const float sc = amax[0] > 0.f ? fp8_max_of<FMT>() / amax[0] : 1.0f;
    for (int64_t c = (int64_t)blockIdx.x * Q_THREADS + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * Q_THREADS) {
        const int64_t r = c / cpr;
        *reinterpret_cast<uint2*>(dst + c * 8) = quant8_fmt<FMT>(*reinterpret_cast<const uint4*>(src + r * ld + (c - r * cpr) * 8), sc);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) scale[0] = sc;
}

template <int FMT, bool WIDE>
__global__ __launch_bounds__(Q_THREADS) void fp8_quant_delayed_fmt_kernel(const unsigned short* __restrict__ src, int64_t rows, int cols,
                                                                           int64_t ld, unsigned char* __restrict__ dst,
                                                                           float* __restrict__ state) {
    __shared__ float sm[Q_THREADS / WAVE];
    constexpr int E = WIDE ? 16 : 8;                                        // elements per thread and trip
    const int cpr = cols / E;
    const int64_t chunks = rows * cpr;
    const float sc = state[0];
    float m = 0.f;
    for (int64_t c = (int64_t)blockIdx.x * Q_THREADS + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * Q_THREADS) {
        const int64_t r = c / cpr;
        const unsigned short* p = src + r * ld + (c - r * cpr) * E;          // (dense rows: r * ld + ... = c * E)
        const uint4 v0 = *reinterpret_cast<const uint4*>(p);
        m = fmaxf(m, amax8(v0));
        if constexpr (WIDE) {
            const uint4 v1 = *reinterpret_cast<const uint4*>(p + 8);
            m = fmaxf(m, amax8(v1));
            if (dst) {
                const uint2 a = quant8_fmt<FMT>(v0, sc), b = quant8_fmt<FMT>(v1, sc);
                *reinterpret_cast<uint4*>(dst + c * 16) = make_uint4(a.x, a.y, b.x, b.y);
            }
        } else {
            if (dst) *reinterpret_cast<uint2*>(dst + c * 8) = quant8_fmt<FMT>(v0, sc);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = sm[0];
#pragma unroll
        for (int i = 1; i < Q_THREADS / WAVE; ++i) t = fmaxf(t, sm[i]);
        state[8 + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(Q_THREADS) void fp8_update_scales_fmt_kernel(float* state, float headroom, float fmax) {
    __shared__ float sm[Q_THREADS / WAVE];
    float* st = state + (size_t)blockIdx.x * Q_STATE;
    float m = 0.f;
    for (int i = threadIdx.x; i < FP8_PARTS; i += Q_THREADS) {
        m = fmaxf(m, st[8 + i]);
        st[8 + i] = 0.f;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = sm[0];
#pragma unroll
        for (int i = 1; i < Q_THREADS / WAVE; ++i) t = fmaxf(t, sm[i]);
        if (t > 0.f && headroom > 0.f) st[0] = fmax / (t * headroom);
    }
}

// ---- byte transpose of an fp8 matrix: dst[c, r] = src[r, c] -- the e4m3 weight mirror W[M,K] -> W^T[K,M] for the fp8
//      input-gradient GEMMs (gx = gy . W as the NT product gy . (W^T)^T).
// A workgroup of 256 threads moves one 128 x 128-byte tile through 16 KiB of LDS, 16-byte global accesses on both sides:
//   in : thread t loads the 16-byte chunks (row q >> 3, chunk q & 7), q = t + 256 j, j < 4 -- 8 consecutive lanes read one 128-byte
//        row segment -- and writes each with one 16-byte LDS write;
//   out: thread t = (rb = t & 7, c4 = t >> 3) reads the dword (4 source columns 4 c4 .. 4 c4 + 3) of the 16 source rows
//        16 rb .. 16 rb + 15, turns the 16 x 4 bytes into 4 x 16 in registers and stores 16 bytes to each of the destination rows
//        4 c4 .. 4 c4 + 3 -- 8 consecutive lanes write one 128-byte row segment.
// LDS image: 128-byte rows with the 16-byte chunk index XOR-ed with bits 4..6 of the row, chunk' = chunk ^ ((row >> 4) & 7) -- the XOR
// swizzle of the programming guide's LDS section ("standard conflict fix: pad each row by one access width, or XOR-swizzle",
// Guideline 4 / T2); padding is no option here, a 4-byte pad would take the 16-byte alignment from the writes.  The transposing read
// is a ds_read_b32: bank = (byte / 4) % 32, conflicts count within a 32-lane half.  A half holds rb = 0..7 and four consecutive c4
// (4 h .. 4 h + 3), and for step i reads row 16 rb + i at dword (c4 ^ (rb << 2)): the low two bits run over the four c4, the upper
// three over the eight rb -- 32 different banks, no conflict.  (Unswizzled, the eight rb of a half would share 4 banks: 8-way.
// The compiler pairs the 16 reads of a thread into 8 ds_read2_b32 -- rows i and i + 1, 128 bytes apart; same bank rule, each half
// of the pair is its own pass.)
// Edges: a chunk is moved only when it lies inside the matrix as a whole (rows, cols multiples of 16: always).
constexpr int T_TILE = 128, T_THREADS = 256;

__device__ __forceinline__ void transpose_tile(const unsigned char* __restrict__ src, int64_t ld_src, int64_t rows, int64_t cols,
                                               unsigned char* __restrict__ dst, int64_t ld_dst, int64_t tile) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[T_TILE * T_TILE];
    const int64_t tiles_c = (cols + T_TILE - 1) / T_TILE;
    const int64_t r0 = (tile / tiles_c) * T_TILE, c0 = (tile % tiles_c) * T_TILE;
    const int t = threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = t + T_THREADS * j, r = q >> 3, k = q & 7;
        if (r0 + r < rows && c0 + k * 16 + 16 <= cols) {
            const uint4 v = *reinterpret_cast<const uint4*>(src + (r0 + r) * ld_src + c0 + k * 16);
            *reinterpret_cast<uint4*>(lds + r * T_TILE + ((k ^ ((r >> 4) & 7)) << 4)) = v;
        }
    }
    __syncthreads();
    const int rb = t & 7, c4 = t >> 3;
    if (r0 + rb * 16 + 16 > rows || c0 + (c4 >> 2) * 16 + 16 > cols) return;   // the 16 rows and the 16-column chunk were loaded as a whole
    unsigned w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = *reinterpret_cast<const unsigned*>(lds + (rb * 16 + i) * T_TILE + ((c4 ^ (rb << 2)) << 2));
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                            // destination row c0 + 4 c4 + j: byte j of the 16 dwords
        unsigned o[4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
            o[m] = ((w[4 * m] >> (8 * j)) & 0xffu) | (((w[4 * m + 1] >> (8 * j)) & 0xffu) << 8) | (((w[4 * m + 2] >> (8 * j)) & 0xffu) << 16) |
                   (((w[4 * m + 3] >> (8 * j)) & 0xffu) << 24);
        *reinterpret_cast<uint4*>(dst + (c0 + c4 * 4 + j) * ld_dst + r0 + rb * 16) = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

__global__ __launch_bounds__(T_THREADS) void fp8_transpose_kernel(const unsigned char* __restrict__ src, int rows, int cols, int64_t ld_src,
                                                                   unsigned char* __restrict__ dst, int64_t ld_dst) {
    transpose_tile(src, ld_src, rows, cols, dst, ld_dst, blockIdx.x);
}

__global__ __launch_bounds__(T_THREADS) void fp8_transpose_seg_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                       const int64_t* __restrict__ src_off, const int64_t* __restrict__ seg_rows,
                                                                       const int64_t* __restrict__ seg_cols, const int64_t* __restrict__ dst_off) {
    const int s = blockIdx.y;
    const int64_t rows = seg_rows[s], cols = seg_cols[s];
    if (rows < 16 || cols < 16) return;
    const int64_t tiles = ((rows + T_TILE - 1) / T_TILE) * ((cols + T_TILE - 1) / T_TILE);
    if ((int64_t)blockIdx.x >= tiles) return;                                 // (uniform over the workgroup)
    transpose_tile(src + src_off[s], cols, rows, cols, dst + dst_off[s], rows, blockIdx.x);
}

}  // namespace kvq

using namespace kvq;

extern "C" {

int kvq_fp8_quantize(const void* x_bf16, int64_t rows, int cols, int64_t ld, void* out_fp8, float* amax, float* scale, void* stream) {
    KVQ_REQUIRE(x_bf16 && out_fp8 && amax && scale && rows > 0 && cols > 0, "kvq_fp8_quantize: bad argument");
    KVQ_REQUIRE(cols % 8 == 0 && ld % 8 == 0 && ld >= cols && (((uintptr_t)x_bf16 | (uintptr_t)out_fp8) & 15) == 0,
                "kvq_fp8_quantize: cols, ld multiples of 8 and 16-byte aligned buffers");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fp8_zero_kernel, dim3(1), dim3(256), 0, st, amax, 1);
    const int64_t chunks = rows * (cols / 8);
    const unsigned grid = (unsigned)((chunks + Q_THREADS * 4 - 1) / (Q_THREADS * 4) > 2048 ? 2048 : (chunks + Q_THREADS * 4 - 1) / (Q_THREADS * 4));
    hipLaunchKernelGGL(fp8_amax_kernel, dim3(grid), dim3(Q_THREADS), 0, st, (const unsigned short*)x_bf16, rows, cols, ld, amax);
    hipLaunchKernelGGL(fp8_quant_kernel, dim3(grid), dim3(Q_THREADS), 0, st, (const unsigned short*)x_bf16, rows, cols, ld, amax,
                       (unsigned char*)out_fp8, scale);
    return check_launch("fp8_quant_kernel");
}

int kvq_fp8_state_floats(void) { return Q_STATE; }

int kvq_fp8_quantize_delayed(const void* x_bf16, int64_t rows, int cols, int64_t ld, void* out_fp8, float* state, void* stream) {
    KVQ_REQUIRE(x_bf16 && out_fp8 && state && rows > 0 && cols > 0, "kvq_fp8_quantize_delayed: bad argument");
    KVQ_REQUIRE(cols % 8 == 0 && ld % 8 == 0 && ld >= cols && (((uintptr_t)x_bf16 | (uintptr_t)out_fp8) & 15) == 0,
                "kvq_fp8_quantize_delayed: cols, ld multiples of 8 and 16-byte aligned buffers");
    hipLaunchKernelGGL(fp8_quant_delayed_kernel, dim3(Q_PARTS), dim3(Q_THREADS), 0, (hipStream_t)stream, (const unsigned short*)x_bf16, rows, cols, ld,
                       (unsigned char*)out_fp8, state);
    return check_launch("fp8_quant_delayed_kernel");
}

int kvq_fp8_update_scales(float* state, int nsites, float headroom, void* stream) {
    KVQ_REQUIRE(state && nsites > 0 && (headroom >= 1.0f || headroom == 0.0f), "kvq_fp8_update_scales: headroom >= 1, or 0 to only clear the amax partials");
    hipLaunchKernelGGL(fp8_update_scales_kernel, dim3((unsigned)nsites), dim3(Q_THREADS), 0, (hipStream_t)stream, state, headroom);
    return check_launch("fp8_update_scales_kernel");
}

int kvq_fp8_quantize_fmt(const void* x_bf16, int64_t rows, int cols, int64_t ld, void* out_fp8, float* amax, float* scale, int fmt,
                         void* stream) {
    KVQ_REQUIRE(fmt == KVQ_FP8_E4M3 || fmt == KVQ_FP8_E5M2, "kvq_fp8_quantize_fmt: fmt must be KVQ_FP8_E4M3 or KVQ_FP8_E5M2, got %d", fmt);
    if (fmt == KVQ_FP8_E4M3) return kvq_fp8_quantize(x_bf16, rows, cols, ld, out_fp8, amax, scale, stream);
    KVQ_REQUIRE(x_bf16 && out_fp8 && amax && scale && rows > 0 && cols > 0, "kvq_fp8_quantize_fmt: bad argument");
    KVQ_REQUIRE(cols % 8 == 0 && ld % 8 == 0 && ld >= cols && (((uintptr_t)x_bf16 | (uintptr_t)out_fp8) & 15) == 0,
                "kvq_fp8_quantize_fmt: cols, ld multiples of 8 and 16-byte aligned buffers");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fp8_zero_kernel, dim3(1), dim3(256), 0, st, amax, 1);
    const int64_t chunks = rows * (cols / 8);
    const unsigned grid = (unsigned)((chunks + Q_THREADS * 4 - 1) / (Q_THREADS * 4) > 2048 ? 2048 : (chunks + Q_THREADS * 4 - 1) / (Q_THREADS * 4));
    hipLaunchKernelGGL(fp8_amax_kernel, dim3(grid), dim3(Q_THREADS), 0, st, (const unsigned short*)x_bf16, rows, cols, ld, amax);
    hipLaunchKernelGGL(fp8_quant_fmt_kernel<KVQ_FP8_E5M2>, dim3(grid), dim3(Q_THREADS), 0, st, (const unsigned short*)x_bf16, rows, cols, ld,
                       amax, (unsigned char*)out_fp8, scale);
    return check_launch("fp8_quant_fmt_kernel");
}

int kvq_fp8_quantize_delayed_fmt(const void* x_bf16, int64_t rows, int cols, int64_t ld, void* out_fp8, float* state, int fmt,
                                 void* stream) {
    KVQ_REQUIRE(fmt == KVQ_FP8_E4M3 || fmt == KVQ_FP8_E5M2, "kvq_fp8_quantize_delayed_fmt: fmt must be KVQ_FP8_E4M3 or KVQ_FP8_E5M2, got %d", fmt);
    KVQ_REQUIRE(x_bf16 && state && rows > 0 && cols > 0, "kvq_fp8_quantize_delayed_fmt: bad argument");
    KVQ_REQUIRE(cols % 8 == 0 && ld % 8 == 0 && ld >= cols && (((uintptr_t)x_bf16 | (uintptr_t)out_fp8) & 15) == 0,
                "kvq_fp8_quantize_delayed_fmt: cols, ld multiples of 8 and 16-byte aligned buffers");
    hipStream_t st = (hipStream_t)stream;
    const unsigned short* x = (const unsigned short*)x_bf16;
    unsigned char* o = (unsigned char*)out_fp8;
    const bool wide = cols % 16 == 0;
    if (fmt == KVQ_FP8_E5M2) {
        if (wide) hipLaunchKernelGGL((fp8_quant_delayed_fmt_kernel<KVQ_FP8_E5M2, true>), dim3(Q_PARTS), dim3(Q_THREADS), 0, st, x, rows, cols, ld, o, state);
        else hipLaunchKernelGGL((fp8_quant_delayed_fmt_kernel<KVQ_FP8_E5M2, false>), dim3(Q_PARTS), dim3(Q_THREADS), 0, st, x, rows, cols, ld, o, state);
    } else {
        if (wide) hipLaunchKernelGGL((fp8_quant_delayed_fmt_kernel<KVQ_FP8_E4M3, true>), dim3(Q_PARTS), dim3(Q_THREADS), 0, st, x, rows, cols, ld, o, state);
        else hipLaunchKernelGGL((fp8_quant_delayed_fmt_kernel<KVQ_FP8_E4M3, false>), dim3(Q_PARTS), dim3(Q_THREADS), 0, st, x, rows, cols, ld, o, state);
    }
    return check_launch("fp8_quant_delayed_fmt_kernel");
}

int kvq_fp8_update_scales_fmt(float* state, int nsites, float headroom, int fmt, void* stream) {
    KVQ_REQUIRE(fmt == KVQ_FP8_E4M3 || fmt == KVQ_FP8_E5M2, "kvq_fp8_update_scales_fmt: fmt must be KVQ_FP8_E4M3 or KVQ_FP8_E5M2, got %d", fmt);
    KVQ_REQUIRE(state && nsites > 0 && (headroom >= 1.0f || headroom == 0.0f),
                "kvq_fp8_update_scales_fmt: headroom >= 1, or 0 to only clear the amax partials");
    hipLaunchKernelGGL(fp8_update_scales_fmt_kernel, dim3((unsigned)nsites), dim3(Q_THREADS), 0, (hipStream_t)stream, state, headroom,
                       fmt == KVQ_FP8_E5M2 ? FP8_MAX_E5M2 : FP8_MAX);
    return check_launch("fp8_update_scales_fmt_kernel");
}

int kvq_fp8_transpose(const void* src8, int rows, int cols, int64_t ld_src, void* dst8, int64_t ld_dst, void* stream) {
    KVQ_REQUIRE(src8 && dst8 && rows > 0 && cols > 0, "kvq_fp8_transpose: bad argument");
    KVQ_REQUIRE(rows % 16 == 0 && cols % 16 == 0 && ld_src % 16 == 0 && ld_dst % 16 == 0 && ld_src >= cols && ld_dst >= rows,
                "kvq_fp8_transpose: rows, cols and both row strides must be multiples of 16 (rows=%d cols=%d), strides covering the rows", rows, cols);
    KVQ_REQUIRE((((uintptr_t)src8 | (uintptr_t)dst8) & 15) == 0, "kvq_fp8_transpose: 16-byte aligned buffers");
    const int64_t tiles = (int64_t)((rows + T_TILE - 1) / T_TILE) * ((cols + T_TILE - 1) / T_TILE);
    KVQ_REQUIRE(tiles < (1ll << 31), "kvq_fp8_transpose: too many tiles");
    hipLaunchKernelGGL(fp8_transpose_kernel, dim3((unsigned)tiles), dim3(T_THREADS), 0, (hipStream_t)stream, (const unsigned char*)src8, rows, cols,
                       ld_src, (unsigned char*)dst8, ld_dst);
    return check_launch("fp8_transpose_kernel");
}

int kvq_fp8_transpose_segments(const void* src8, void* dst8, const int64_t* src_off, const int64_t* seg_rows, const int64_t* seg_cols,
                               const int64_t* dst_off, int nseg, int64_t max_tiles, void* stream) {
    KVQ_REQUIRE(src8 && dst8 && src_off && seg_rows && seg_cols && dst_off, "kvq_fp8_transpose_segments: null pointer");
    KVQ_REQUIRE(nseg > 0 && nseg < 65536 && max_tiles > 0 && max_tiles < (1ll << 31), "kvq_fp8_transpose_segments: 1..65535 segments, max_tiles > 0");
    KVQ_REQUIRE((((uintptr_t)src8 | (uintptr_t)dst8) & 15) == 0, "kvq_fp8_transpose_segments: 16-byte aligned buffers");
    hipLaunchKernelGGL(fp8_transpose_seg_kernel, dim3((unsigned)max_tiles, (unsigned)nseg), dim3(T_THREADS), 0, (hipStream_t)stream,
                       (const unsigned char*)src8, (unsigned char*)dst8, src_off, seg_rows, seg_cols, dst_off);
    return check_launch("fp8_transpose_seg_kernel");
}

static int quantize_segments_impl(const void* src_bf16, const int64_t* seg_off, const int64_t* seg_n, int nseg, int64_t max_seg_n, void* dst_fp8,
                                  float* amax, float* scale, const unsigned long long* step, int period, void* stream);

int kvq_fp8_quantize_segments(const void* src_bf16, const int64_t* seg_off, const int64_t* seg_n, int nseg, int64_t max_seg_n, void* dst_fp8,
                              float* amax, float* scale, void* stream) {
    return quantize_segments_impl(src_bf16, seg_off, seg_n, nseg, max_seg_n, dst_fp8, amax, scale, nullptr, 1, stream);
}

int kvq_fp8_quantize_segments_periodic(const void* src_bf16, const int64_t* seg_off, const int64_t* seg_n, int nseg, int64_t max_seg_n,
                                       void* dst_fp8, float* amax, float* scale, const void* step_count_u64, int period, void* stream) {
    KVQ_REQUIRE(step_count_u64 && (period >= 1 || period < -1), "kvq_fp8_quantize_segments_periodic: a device step counter and |period| >= 1");
    return quantize_segments_impl(src_bf16, seg_off, seg_n, nseg, max_seg_n, dst_fp8, amax, scale, (const unsigned long long*)step_count_u64,
                                  period, stream);
}

static int quantize_segments_impl(const void* src_bf16, const int64_t* seg_off, const int64_t* seg_n, int nseg, int64_t max_seg_n, void* dst_fp8,
                                  float* amax, float* scale, const unsigned long long* step, int period, void* stream) {
    KVQ_REQUIRE(src_bf16 && seg_off && seg_n && dst_fp8 && amax && scale && nseg > 0 && max_seg_n > 0, "kvq_fp8_quantize_segments: bad argument");
    KVQ_REQUIRE((((uintptr_t)src_bf16 | (uintptr_t)dst_fp8) & 15) == 0, "kvq_fp8_quantize_segments: 16-byte aligned buffers");
    hipStream_t st = (hipStream_t)stream;
    const int gate = period < 0 ? -period : period;          // period < 0: also the conversion pass runs on refresh steps only
    hipLaunchKernelGGL(fp8_zero_kernel, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, st, amax, nseg, step, gate);
    const int64_t chunks = max_seg_n / 8;
    unsigned gx = (unsigned)((chunks + Q_THREADS * 8 - 1) / (Q_THREADS * 8));
    gx = gx < 1 ? 1 : (gx > 256 ? 256 : gx);
    hipLaunchKernelGGL(fp8_seg_amax_kernel, dim3(gx, (unsigned)nseg), dim3(Q_THREADS), 0, st, (const unsigned short*)src_bf16, seg_off, seg_n, amax,
                       step, gate);
    hipLaunchKernelGGL(fp8_seg_quant_kernel, dim3(gx, (unsigned)nseg), dim3(Q_THREADS), 0, st, (const unsigned short*)src_bf16, seg_off, seg_n, amax,
                       (unsigned char*)dst_fp8, scale, step, period);
    return check_launch("fp8_seg_quant_kernel");
}

}  // extern "C"
