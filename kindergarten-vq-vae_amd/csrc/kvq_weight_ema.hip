// kvq_weight_ema.hip -- exponential moving average of the trained weights, kept inside the optimiser step (gfx950).
//
// TrainEngine(weight_ema=decay) keeps, beside the f32 master copy of every trainable parameter, an f32 average of what the
// optimiser left there step after step, and evaluates / checkpoints under it (weight_ema_applied()).  The parameters are views
// of one flat buffer that Adam writes through raw pointers inside a replayed hipGraph, so the average is built the same way:
//     kvq_weight_ema_update    ema = p (first update: a store, ema is NOT read), ema = d ema + (1 - d) p (the others), with
//                              d = min(decay, (1 + t) / (10 + t)) from the update count t read on the device
//     kvq_weight_ema_advance   one thread: last_decay = the d this step used (0 for the storing step), updates += 1
//     kvq_weight_ema_swap      p <-> ema, element by element, and the bf16 shadow of the new p: evaluation under the average
// Which of the two forms an update launch takes is read from the 16-byte state, so one captured chain serves every step.  With
// a gradient guard whose skip flag is set both kernels return before their first store: the Adam kernels stored nothing either,
// and the average of a skipped step does not move.
//
// The update is a stream: 4 bytes of p and 4 of ema read (not on the first update), 4 written.  16-byte accesses per lane, two
// chunks in flight per thread, a grid-stride loop over at most EMA_MAX_BLOCKS workgroups, the last n % 4 elements one by one.
// Elementwise, no atomics: the same bits on every run.  The arithmetic is f64 -- two products, one sum, each rounded on its own
// (the library is built with -ffp-contract=off and the pragma below says it again for this file: d * ema needs 77 bits, an FMA
// would keep them) -- and one final rounding to f32: with d = 0.9999, 1 - d in f32 is off by 2.4e-8 relative to ema's weight,
// which a run of 1e5 steps would carry into every element.  Six f64 operations per 12 bytes stay far below the memory time.
#include "kvq_common.h"

#pragma clang fp contract(off)

namespace kvq {

constexpr int EMA_THREADS = 256;
constexpr int EMA_MAX_BLOCKS = 2048;   // 8 workgroups per CU of an MI355X; the grid-stride loop takes what is beyond 2048 * 256 * 4 elements

struct WeightEmaState {
    unsigned long long updates;   // updates applied so far (skipped steps do not count)
    float last_decay;             // the d of the last applied update; 0 for the storing one
    uint32_t pad;
};
static_assert(sizeof(WeightEmaState) == 16, "the weight-EMA state is 16 bytes (include/kvq.h)");

// the warm-up schedule: the average of the first steps follows the weights closely, min(decay, (1 + t) / (10 + t)) reaches decay
// at t = (10 decay - 1) / (1 - decay)
__device__ __forceinline__ double ema_decay_at(unsigned long long t, float decay) {
    const double w = (1.0 + (double)t) / (10.0 + (double)t), d = (double)decay;
    return d < w ? d : w;
}

__device__ __forceinline__ float ema1(float e, float p, double d, double omd) {
    const double a = d * (double)e, b = omd * (double)p;
    return (float)(a + b);
}

// FIRST: store (ema is not read).  Uniform over the launch.
template <bool FIRST>
__device__ __forceinline__ void ema_chunk(const f32x4 p, float* __restrict__ ema, int64_t e, double d, double omd) {
    f32x4 s = p;
    if (!FIRST) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(ema + e);
        s.x = ema1(a.x, p.x, d, omd); s.y = ema1(a.y, p.y, d, omd); s.z = ema1(a.z, p.z, d, omd); s.w = ema1(a.w, p.w, d, omd);
    }
    *reinterpret_cast<f32x4*>(ema + e) = s;
}

// chunk i = elements [4 i, 4 i + 4); thread t of the grid takes chunks t, t + T, t + 2T, ... (T = gridDim.x * 256), two per pass
template <bool FIRST>
__device__ __forceinline__ void ema_body(const float* __restrict__ p, float* __restrict__ ema, int64_t n, double d, double omd) {
    const int64_t n4 = n >> 2;
    const int64_t T = (int64_t)gridDim.x * EMA_THREADS;
    int64_t i = (int64_t)blockIdx.x * EMA_THREADS + threadIdx.x;
    for (; i + T < n4; i += 2 * T) {
        const f32x4 p0 = *reinterpret_cast<const f32x4*>(p + 4 * i), p1 = *reinterpret_cast<const f32x4*>(p + 4 * (i + T));
        ema_chunk<FIRST>(p0, ema, 4 * i, d, omd);
        ema_chunk<FIRST>(p1, ema, 4 * (i + T), d, omd);
    }
    if (i < n4) ema_chunk<FIRST>(*reinterpret_cast<const f32x4*>(p + 4 * i), ema, 4 * i, d, omd);
    const int64_t e = 4 * n4 + threadIdx.x;                                // the last n % 4 elements, one per thread of workgroup 0
    if (blockIdx.x == 0 && threadIdx.x < 4 && e < n) ema[e] = FIRST ? p[e] : ema1(ema[e], p[e], d, omd);
}

__global__ __launch_bounds__(EMA_THREADS) void weight_ema_update_kernel(const float* __restrict__ p, float* __restrict__ ema, int64_t n,
                                                                        float decay, const WeightEmaState* __restrict__ st,
                                                                        const GradGuard* __restrict__ guard) {
    if (guard && guard->skip) return;                                      // a skipped step stored nothing: the average stays (uniform)
    const unsigned long long t = st->updates;                              // (uniform)
    if (t == 0) {
        ema_body<true>(p, ema, n, 0.0, 1.0);
    } else {
        const double d = ema_decay_at(t, decay);
        ema_body<false>(p, ema, n, d, 1.0 - d);
    }
}

__global__ void weight_ema_advance_kernel(WeightEmaState* st, float decay, const GradGuard* guard) {
    if (guard && guard->skip) return;
    const unsigned long long t = st->updates;
    st->last_decay = t == 0 ? 0.f : (float)ema_decay_at(t, decay);
    st->updates = t + 1ull;
}

// p <-> ema; the bf16 shadow of the new p with the rounding of adam_kernel's shadow store (IO<KVQ_BF16>::store4 / store1)
__global__ __launch_bounds__(EMA_THREADS) void weight_ema_swap_kernel(float* __restrict__ p, float* __restrict__ ema,
                                                                      unsigned short* __restrict__ shadow, int64_t n) {
    const int64_t n4 = n >> 2;
    const int64_t T = (int64_t)gridDim.x * EMA_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * EMA_THREADS + threadIdx.x; i < n4; i += T) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p + 4 * i), b = *reinterpret_cast<const f32x4*>(ema + 4 * i);
        *reinterpret_cast<f32x4*>(p + 4 * i) = b;
        *reinterpret_cast<f32x4*>(ema + 4 * i) = a;
        if (shadow) IO<KVQ_BF16>::store4(shadow, (size_t)(4 * i), b);
    }
    const int64_t e = 4 * n4 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < 4 && e < n) {
        const float a = p[e], b = ema[e];
        p[e] = b;
        ema[e] = a;
        if (shadow) IO<KVQ_BF16>::store1(shadow, (size_t)e, b);
    }
}

static inline unsigned ema_blocks(int64_t n) {
    const int64_t n4 = n >> 2;
    const int64_t blocks = (n4 + EMA_THREADS - 1) / EMA_THREADS;
    return (unsigned)(blocks < 1 ? 1 : (blocks > EMA_MAX_BLOCKS ? EMA_MAX_BLOCKS : blocks));
}

static inline bool overlap(uintptr_t a, uintptr_t a_bytes, uintptr_t b, uintptr_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

}  // namespace kvq

using namespace kvq;

extern "C" {

int kvq_weight_ema_update(const float* p, float* ema, int64_t n, float decay, const void* ema_state, const void* guard, void* stream) {
    KVQ_REQUIRE(p && ema && ema_state, "kvq_weight_ema_update: null pointer argument");
    KVQ_REQUIRE(n >= 1, "kvq_weight_ema_update: n < 1 (n=%lld)", (long long)n);
    KVQ_REQUIRE(decay > 0.f && decay < 1.f, "kvq_weight_ema_update: decay outside (0, 1) (decay=%g)", (double)decay);
    KVQ_REQUIRE((((uintptr_t)p | (uintptr_t)ema) & 15) == 0 && (((uintptr_t)ema_state | (uintptr_t)guard) & 7) == 0,
                "kvq_weight_ema_update: 16-byte aligned parameters and average (8-byte aligned state and guard) required");
    KVQ_REQUIRE(!overlap((uintptr_t)p, (uintptr_t)n * 4, (uintptr_t)ema, (uintptr_t)n * 4),
                "kvq_weight_ema_update: the parameters and their average overlap");
    hipLaunchKernelGGL(weight_ema_update_kernel, dim3(ema_blocks(n)), dim3(EMA_THREADS), 0, (hipStream_t)stream, p, ema, n, decay,
                       reinterpret_cast<const WeightEmaState*>(ema_state), reinterpret_cast<const GradGuard*>(guard));
    return check_launch("weight_ema_update_kernel");
}

int kvq_weight_ema_advance(void* ema_state, float decay, const void* guard, void* stream) {
    KVQ_REQUIRE(ema_state, "kvq_weight_ema_advance: null weight-EMA state");
    KVQ_REQUIRE(decay > 0.f && decay < 1.f, "kvq_weight_ema_advance: decay outside (0, 1) (decay=%g)", (double)decay);
    KVQ_REQUIRE((((uintptr_t)ema_state | (uintptr_t)guard) & 7) == 0, "kvq_weight_ema_advance: 8-byte aligned state and guard required");
    hipLaunchKernelGGL(weight_ema_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (WeightEmaState*)ema_state, decay,
                       reinterpret_cast<const GradGuard*>(guard));
    return check_launch("weight_ema_advance_kernel");
}

int kvq_weight_ema_swap(float* p, float* ema, void* shadow_bf16, int64_t n, void* stream) {
    KVQ_REQUIRE(p && ema, "kvq_weight_ema_swap: null pointer argument");
    KVQ_REQUIRE(n >= 1, "kvq_weight_ema_swap: n < 1 (n=%lld)", (long long)n);
    KVQ_REQUIRE((((uintptr_t)p | (uintptr_t)ema) & 15) == 0 && ((uintptr_t)shadow_bf16 & 7) == 0,
                "kvq_weight_ema_swap: 16-byte aligned parameters and average (8-byte aligned bf16 shadow) required");
    const uintptr_t bytes = (uintptr_t)n * 4;
    KVQ_REQUIRE(p != ema && !overlap((uintptr_t)p, bytes, (uintptr_t)ema, bytes), "kvq_weight_ema_swap: the parameters and their average overlap");
    KVQ_REQUIRE(!shadow_bf16 || (!overlap((uintptr_t)shadow_bf16, bytes / 2, (uintptr_t)p, bytes) &&
                                 !overlap((uintptr_t)shadow_bf16, bytes / 2, (uintptr_t)ema, bytes)),
                "kvq_weight_ema_swap: the bf16 shadow overlaps the parameters or their average");
    hipLaunchKernelGGL(weight_ema_swap_kernel, dim3(ema_blocks(n)), dim3(EMA_THREADS), 0, (hipStream_t)stream, p, ema,
                       reinterpret_cast<unsigned short*>(shadow_bf16), n);
    return check_launch("weight_ema_swap_kernel");
}

}  // extern "C"
