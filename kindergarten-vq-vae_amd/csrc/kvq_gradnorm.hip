// kvq_gradnorm.hip -- the global gradient norm of a training step and the guard the Adam kernels read (gfx950).
//
// Between backward and Adam the step may look at its gradients once (TrainEngine(max_grad_norm=...)):
//     kvq_grad_sumsq_partial     sum of squares of one piece of the gradient -> GN_PARTIALS f64 partial sums
//     kvq_grad_guard_finalize    all partials -> the guard state: norm, the clipping coefficient of
//                                torch.nn.utils.clip_grad_norm_, and the skip flag of a step whose gradient is not finite
// and kvq_adam_step_guarded* (csrc/kvq_adam.hip) multiply the gradient by guard->coef or, with guard->skip set, store nothing.
// Everything is a kernel launch on the step's stream reading and writing device memory: no host round trip, nothing a captured
// step would have to patch.
//
// The reduction is HBM-bound (2 bytes read per bf16 gradient, nothing written but 16 KiB of partials): 16-byte loads per lane,
// four of them in flight per thread, a grid-stride loop shaped like adam_kernel's.  It is deterministic: a FIXED grid of
// GN_PARTIALS workgroups whatever the device, so element -> thread -> workgroup -> partial depends on n alone, and no
// floating-point atomic anywhere.  A thread squares and adds the 8 elements of one 16-byte chunk in f32 (8 products of bf16
// or f32 values; the overflow of an f32 square gives inf, which is what the guard wants to see) and accumulates the chunk
// sums in f64, as the wave, the workgroup and kvq_grad_guard_finalize do: the only f32 roundings are those 8 additions.
#include "kvq_common.h"

namespace kvq {

constexpr int GN_THREADS = 256;
constexpr int GN_PARTIALS = 2048;      // workgroups = partial sums per call: 8 per CU of an MI355X (kvq_grad_sumsq_partials())
constexpr int GN_UNROLL = 4;

__device__ __forceinline__ float sumsq8(const f32x8& x) {
    const f32x4 a = x.lo * x.lo, b = x.hi * x.hi;
    return ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w));
}

// sum over the workgroup in a fixed order: xor-butterfly inside each wave, then waves 0..3 in order.  Thread 0 holds the result.
__device__ __forceinline__ double block_sum_f64(double v) {
    __shared__ double wave_part[GN_THREADS / WAVE];
    v = wave_sum_f64(v);
    if ((threadIdx.x & (WAVE - 1)) == 0) wave_part[threadIdx.x / WAVE] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < GN_THREADS / WAVE; ++w) s += wave_part[w];
    }
    return s;
}

// chunk i = elements [8 i, 8 i + 8); thread t of the grid takes chunks t, t + T, t + 2T, ... (T = GN_PARTIALS * GN_THREADS)
template <int DT>
__global__ __launch_bounds__(GN_THREADS) void grad_sumsq_kernel(const void* __restrict__ g, int64_t n, double* __restrict__ partials) {
    const int64_t n8 = n >> 3;
    const int64_t T = (int64_t)GN_PARTIALS * GN_THREADS;
    double acc = 0.0;
    int64_t i = (int64_t)blockIdx.x * GN_THREADS + threadIdx.x;
    for (; i + (GN_UNROLL - 1) * T < n8; i += GN_UNROLL * T) {
        f32x8 x[GN_UNROLL];
#pragma unroll
        for (int u = 0; u < GN_UNROLL; ++u) x[u] = IO<DT>::load8(g, (size_t)(8 * (i + u * T)));
#pragma unroll
        for (int u = 0; u < GN_UNROLL; ++u) acc += (double)sumsq8(x[u]);
    }
    for (; i < n8; i += T) acc += (double)sumsq8(IO<DT>::load8(g, (size_t)(8 * i)));
    if (blockIdx.x == 0 && threadIdx.x == 0) {                           // the last n % 8 elements, one at a time
        for (int64_t e = 8 * n8; e < n; ++e) {
            const float x = IO<DT>::load1(g, (size_t)e);
            acc += (double)(x * x);
        }
    }
    const double s = block_sum_f64(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// one workgroup: thread t adds partials t, t + 256, ... in that order, then the fixed order of block_sum_f64
__global__ __launch_bounds__(GN_THREADS) void grad_guard_finalize_kernel(const double* __restrict__ partials, int n_total, float max_norm,
                                                                         GradGuard* __restrict__ guard) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_total; i += GN_THREADS) acc += partials[i];
    const double sumsq = block_sum_f64(acc);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(sumsq);
    guard->sumsq = sumsq;
    guard->norm = norm;
    if (sumsq - sumsq == 0.0) {                                          // finite (inf - inf and NaN - NaN are NaN)
        const float c = max_norm / (norm + 1e-6f);                       // torch.nn.utils.clip_grad_norm_'s clip_coef ...
        guard->coef = c < 1.0f ? c : 1.0f;                               // ... clamped to 1 (max_norm = +inf: 1, measure and guard only)
        guard->skip = 0u;
    } else {
        guard->coef = 0.0f;
        guard->skip = 1u;
        guard->skipped += 1ull;
    }
}

}  // namespace kvq

using namespace kvq;

extern "C" {

int kvq_grad_sumsq_partials(void) { return GN_PARTIALS; }

int kvq_grad_sumsq_partial(const void* g, int64_t n, int grad_dtype, double* partials, int n_partials, void* stream) {
    KVQ_REQUIRE(g && partials && n >= 1, "kvq_grad_sumsq_partial: null pointer or n < 1 (n=%lld)", (long long)n);
    KVQ_REQUIRE(n_partials == GN_PARTIALS, "kvq_grad_sumsq_partial: n_partials must be kvq_grad_sumsq_partials() = %d, got %d", GN_PARTIALS,
                n_partials);
    KVQ_REQUIRE(grad_dtype == KVQ_F32 || grad_dtype == KVQ_BF16, "kvq_grad_sumsq_partial: unsupported gradient dtype %d", grad_dtype);
    KVQ_REQUIRE(((uintptr_t)g & 15) == 0 && ((uintptr_t)partials & 7) == 0, "kvq_grad_sumsq_partial: 16-byte aligned gradient required");
    hipStream_t st = (hipStream_t)stream;
    if (grad_dtype == KVQ_F32)
        hipLaunchKernelGGL(grad_sumsq_kernel<KVQ_F32>, dim3(GN_PARTIALS), dim3(GN_THREADS), 0, st, g, n, partials);
    else
        hipLaunchKernelGGL(grad_sumsq_kernel<KVQ_BF16>, dim3(GN_PARTIALS), dim3(GN_THREADS), 0, st, g, n, partials);
    return check_launch("grad_sumsq_kernel");
}

int kvq_grad_guard_finalize(const double* partials, int n_total, float max_norm, void* guard, void* stream) {
    KVQ_REQUIRE(partials && guard, "kvq_grad_guard_finalize: null pointer argument");
    KVQ_REQUIRE(n_total >= GN_PARTIALS && n_total % GN_PARTIALS == 0,
                "kvq_grad_guard_finalize: n_total must be a positive multiple of kvq_grad_sumsq_partials() = %d, got %d", GN_PARTIALS, n_total);
    KVQ_REQUIRE(max_norm > 0.0f, "kvq_grad_guard_finalize: max_norm must be > 0 (+inf: measure and guard only), got %g", (double)max_norm);
    KVQ_REQUIRE(((uintptr_t)partials & 7) == 0 && ((uintptr_t)guard & 7) == 0, "kvq_grad_guard_finalize: 8-byte aligned buffers required");
    hipLaunchKernelGGL(grad_guard_finalize_kernel, dim3(1), dim3(GN_THREADS), 0, (hipStream_t)stream, partials, n_total, max_norm,
                       (GradGuard*)guard);
    return check_launch("grad_guard_finalize_kernel");
}

}  // extern "C"
