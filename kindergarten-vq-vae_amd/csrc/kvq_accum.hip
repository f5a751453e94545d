// kvq_accum.hip -- gradient accumulation over the micro-batches of one optimiser step (gfx950).
//
// TrainEngine(grad_accum=A) runs forward and backward A times before Adam runs once, on the MEAN of the A gradients: the
// (loss / A).backward() x A, opt.step() idiom.  The flat gradient buffer is bf16 and is overwritten by every backward, so the sum
// lives in an f32 accumulator of its own:
//     kvq_grad_accumulate    acc = g (first micro-step of a cycle: a store, acc is NOT read), acc += g (the others), and on the
//                            last micro-step acc = (acc + g) * (1 / A): what Adam and the gradient-norm kernels then read as a
//                            KVQ_F32 gradient with grad_scale 1
//     kvq_accum_advance      one thread: tick += 1, micro = (micro + 1) mod A
// Which of the three a launch does is read on the device from the 16-byte accumulation state, so one captured chain of launches
// serves every position of the cycle but the last.  `tick` is the first word of the state: kvq_set_seed_offset points the dropout
// seeds at it, and the A micro-steps of one optimiser step draw A different sets of masks.
//
// The kernel is a stream: 2 (bf16) or 4 (f32) bytes read per gradient element, 4 bytes of accumulator read (not on the first
// micro-step) and 4 written.  16-byte accesses per lane (IO<DT>::load8, two f32x4 for the accumulator), two chunks in flight per
// thread, a grid-stride loop over at most ACC_MAX_BLOCKS workgroups.  Elementwise, no atomics: the same bits on every run.  The add
// and the multiply are two roundings: (acc + g) * c holds no multiply-then-add a compiler could fuse, and the library is built with
// -ffp-contract=off.  (__fadd_rn / __fmul_rn only spell that out: in this HIP they are plain + and * and promise nothing about
// contraction -- do not lean on them where an FMA could form.)
#include "kvq_common.h"

namespace kvq {

constexpr int ACC_THREADS = 256;
constexpr int ACC_MAX_BLOCKS = 2048;   // 8 workgroups per CU of an MI355X; the grid-stride loop takes what is beyond 2048 * 256 * 8 elements

struct AccumState {
    unsigned long long tick;    // micro-steps finished so far, never reset: the addend of the dropout seeds of an accumulating engine
    uint32_t micro, pad;        // tick mod A: the position inside the current cycle
};
static_assert(sizeof(AccumState) == 16, "the accumulation state is 16 bytes (include/kvq.h)");

// FIRST: store (acc is not read); LAST: the sum becomes the mean.  Both are uniform over the launch.
template <bool FIRST>
__device__ __forceinline__ f32x4 accum4(const float* __restrict__ acc, f32x4 g, bool last, float inv_a) {
    f32x4 s = g;
    if (!FIRST) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(acc);
        s.x = __fadd_rn(a.x, g.x); s.y = __fadd_rn(a.y, g.y); s.z = __fadd_rn(a.z, g.z); s.w = __fadd_rn(a.w, g.w);
    }
    if (last) { s.x = __fmul_rn(s.x, inv_a); s.y = __fmul_rn(s.y, inv_a); s.z = __fmul_rn(s.z, inv_a); s.w = __fmul_rn(s.w, inv_a); }
    return s;
}

template <bool FIRST>
__device__ __forceinline__ void accum_chunk(const f32x8& g, float* __restrict__ acc, int64_t e, bool last, float inv_a) {
    const f32x4 lo = accum4<FIRST>(acc + e, g.lo, last, inv_a), hi = accum4<FIRST>(acc + e + 4, g.hi, last, inv_a);
    *reinterpret_cast<f32x4*>(acc + e) = lo;
    *reinterpret_cast<f32x4*>(acc + e + 4) = hi;
}

// chunk i = elements [8 i, 8 i + 8); thread t of the grid takes chunks t, t + T, t + 2T, ... (T = gridDim.x * 256), two per pass
template <int DT, bool FIRST>
__device__ __forceinline__ void accum_body(const void* __restrict__ g, int64_t n, float* __restrict__ acc, bool last, float inv_a) {
    const int64_t n8 = n >> 3;
    const int64_t T = (int64_t)gridDim.x * ACC_THREADS;
    int64_t i = (int64_t)blockIdx.x * ACC_THREADS + threadIdx.x;
    for (; i + T < n8; i += 2 * T) {
        const f32x8 g0 = IO<DT>::load8(g, (size_t)(8 * i)), g1 = IO<DT>::load8(g, (size_t)(8 * (i + T)));
        accum_chunk<FIRST>(g0, acc, 8 * i, last, inv_a);
        accum_chunk<FIRST>(g1, acc, 8 * (i + T), last, inv_a);
    }
    if (i < n8) accum_chunk<FIRST>(IO<DT>::load8(g, (size_t)(8 * i)), acc, 8 * i, last, inv_a);
    const int64_t e = 8 * n8 + threadIdx.x;                               // the last n % 8 elements, one per thread of workgroup 0
    if (blockIdx.x == 0 && threadIdx.x < 8 && e < n) {
        const float x = IO<DT>::load1(g, (size_t)e);
        float s = FIRST ? x : __fadd_rn(acc[e], x);
        if (last) s = __fmul_rn(s, inv_a);
        acc[e] = s;
    }
}

template <int DT>
__global__ __launch_bounds__(ACC_THREADS) void grad_accumulate_kernel(const void* __restrict__ g, int64_t n, float* __restrict__ acc,
                                                                      const AccumState* __restrict__ st, int A, float inv_a) {
    const uint32_t micro = st->micro;                                     // (uniform)
    const bool last = micro + 1 == (uint32_t)A;
    if (micro == 0)
        accum_body<DT, true>(g, n, acc, last, inv_a);
    else
        accum_body<DT, false>(g, n, acc, last, inv_a);
}

__global__ void accum_advance_kernel(AccumState* st, int A) {
    const uint32_t next = st->micro + 1;
    st->tick += 1ull;
    st->micro = next == (uint32_t)A ? 0u : next;
}

}  // namespace kvq

using namespace kvq;

extern "C" {

int kvq_grad_accumulate(const void* g, int64_t n, int grad_dtype, float* acc, const void* accum_state, int A, void* stream) {
    KVQ_REQUIRE(g && acc && accum_state, "kvq_grad_accumulate: null pointer argument");
    KVQ_REQUIRE(n >= 1, "kvq_grad_accumulate: n < 1 (n=%lld)", (long long)n);
    KVQ_REQUIRE(A >= 1, "kvq_grad_accumulate: A < 1 (A=%d)", A);
    KVQ_REQUIRE(grad_dtype == KVQ_F32 || grad_dtype == KVQ_BF16, "kvq_grad_accumulate: unsupported gradient dtype %d", grad_dtype);
    KVQ_REQUIRE((((uintptr_t)g | (uintptr_t)acc) & 15) == 0 && ((uintptr_t)accum_state & 7) == 0,
                "kvq_grad_accumulate: 16-byte aligned gradient and accumulator (8-byte aligned state) required");
    const int64_t n8 = n >> 3;
    int64_t blocks = (n8 + ACC_THREADS - 1) / ACC_THREADS;
    blocks = blocks < 1 ? 1 : (blocks > ACC_MAX_BLOCKS ? ACC_MAX_BLOCKS : blocks);
    const float inv_a = (float)(1.0 / (double)A);
    hipStream_t st = (hipStream_t)stream;
    const AccumState* as = reinterpret_cast<const AccumState*>(accum_state);
    if (grad_dtype == KVQ_F32)
        hipLaunchKernelGGL(grad_accumulate_kernel<KVQ_F32>, dim3((unsigned)blocks), dim3(ACC_THREADS), 0, st, g, n, acc, as, A, inv_a);
    else
        hipLaunchKernelGGL(grad_accumulate_kernel<KVQ_BF16>, dim3((unsigned)blocks), dim3(ACC_THREADS), 0, st, g, n, acc, as, A, inv_a);
    return check_launch("grad_accumulate_kernel");
}

int kvq_accum_advance(void* accum_state, int A, void* stream) {
    KVQ_REQUIRE(accum_state, "kvq_accum_advance: null accumulation state");
    KVQ_REQUIRE(A >= 1, "kvq_accum_advance: A < 1 (A=%d)", A);
    KVQ_REQUIRE(((uintptr_t)accum_state & 7) == 0, "kvq_accum_advance: 8-byte aligned state required");
    hipLaunchKernelGGL(accum_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (AccumState*)accum_state, A);
    return check_launch("accum_advance_kernel");
}

}  // extern "C"
