// kvq_vq_revive.hip -- codebook revival: a code that won no token for `revive_after` training steps restarts from a random
// encoder output of the current batch (gfx950).  Extension, off by default (VectorQuantizer(revive_after=...)); contract in include/kvq.h.
//
// A training step runs, on its own stream and with no host round trip (so a captured step replays it unchanged):
//     kvq_vq_usage_flags      idx -> used[G, K]: which codes won a token in this batch
//     kvq_vq_revive_select    used -> idle; for every code that is now dead: the donor token's row -> rows[G, K, D]
//     kvq_vq_revive_apply     after the codebook's own update: rows -> E (and the EMA statistics), Adam moments of the row to zero
// Between the three the data-parallel caller all-reduces `used` (MAX) and `rows` (SUM: one owner rank wrote the row, the others zeros).
//
// Latency-sized streaming kernels: the index scan reads 64 KB that sit in L2, a dead code moves one row.  Deterministic: no float
// atomics (no atomics at all), every element of `used` has one writer, a code has one wave, the count is one workgroup's fixed tree.
#include "kvq_common.h"

namespace kvq {

constexpr int RV_THREADS = 256;
constexpr int RV_SLICE = 64;                        // codes of one codebook owned by a workgroup of kvq_vq_usage_flags
constexpr int RV_WAVES = RV_THREADS / WAVE;         // codes per workgroup of select / apply: one wave each
constexpr unsigned RV_SITE = 0x52455649u;           // "REVI": the Philox site of the donor draw; dropout sites are a small counter

struct ReviveCounter {
    uint32_t last, pad;           // codes revived by the last kvq_vq_revive_apply
    unsigned long long total;     // codes revived so far
};
static_assert(sizeof(ReviveCounter) == 16, "the revival counter is 16 bytes (include/kvq.h)");

// grid (ceil(K / RV_SLICE), G): the workgroup scans ALL N indices of its codebook and keeps a flag per owned code in LDS (the
// stores of one flag all write 1: no atomic needed), then writes its slice of used -- every element of used, by one launch, no clear
__global__ __launch_bounds__(RV_THREADS) void usage_flags_kernel(const int64_t* __restrict__ idx, long long N, int K,
                                                                 int32_t* __restrict__ used) {
    __shared__ int flag[RV_SLICE];
    const int g = blockIdx.y;
    const long long k0 = (long long)blockIdx.x * RV_SLICE;
    if (threadIdx.x < RV_SLICE) flag[threadIdx.x] = 0;
    __syncthreads();
    const int64_t* row = idx + (size_t)g * (size_t)N;
    for (long long n = threadIdx.x; n < N; n += RV_THREADS) {
        const long long d = (long long)row[n] - k0;                     // an index outside [0, K) lands in no workgroup's slice
        if (d >= 0 && d < RV_SLICE && k0 + d < K) flag[d] = 1;
    }
    __syncthreads();
    if (threadIdx.x < RV_SLICE && k0 + threadIdx.x < K) used[(size_t)g * K + k0 + threadIdx.x] = flag[threadIdx.x];
}

// one wave per code c = g K + k.  VEC: rows of z are whole 16-byte chunks (pitch D * sizeof(elem) a multiple of 16)
template <int DT, bool VEC>
__global__ __launch_bounds__(RV_THREADS) void revive_select_kernel(const void* __restrict__ z, const int32_t* __restrict__ used, long long N,
                                                                   int K, int D, int GK, int revive_after, unsigned long long seed,
                                                                   const unsigned long long* __restrict__ seed_off, int rank, int world,
                                                                   int32_t* __restrict__ idle, float* __restrict__ rows) {
    const int c = blockIdx.x * RV_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & (WAVE - 1);
    if (c >= GK) return;
    const int32_t before = idle[c];
    const int32_t now = used[c] ? 0 : (before == INT32_MAX ? INT32_MAX : before + 1);
    if (lane == 0) idle[c] = now;
    if (now < revive_after) return;                                      // not dead: nothing else is read or written
    if (seed_off) seed += *seed_off;
    const U4 r = drop_bits(seed, RV_SITE, (unsigned long long)c);
    const bool mine = (int)(r.y % (unsigned)world) == rank;
    const unsigned long long n = ((unsigned long long)r.x * (unsigned long long)N) >> 32;        // < N
    const size_t src = ((size_t)(c / K) * (size_t)N + (size_t)n) * (size_t)D;                    // z[g, n, 0]
    float* dst = rows + (size_t)c * D;
    if (VEC) {
        constexpr int E = 16 / IO<DT>::bytes;                            // elements of a 16-byte chunk: 4 f32 or 8 bf16
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        for (int d = lane * E; d < D; d += WAVE * E) {
            if (DT == KVQ_F32) {
                *reinterpret_cast<f32x4*>(dst + d) = mine ? IO<DT>::load4(z, src + d) : zero;
            } else {
                f32x8 v = {zero, zero};
                if (mine) v = IO<DT>::load8(z, src + d);
                *reinterpret_cast<f32x4*>(dst + d) = v.lo;
                *reinterpret_cast<f32x4*>(dst + d + 4) = v.hi;
            }
        }
    } else {
        for (int d = lane; d < D; d += WAVE) dst[d] = mine ? IO<DT>::load1(z, src + d) : 0.f;
    }
}

// one workgroup: last = number of dead codes (idle >= revive_after), total += last.  Runs BEFORE revive_apply_kernel clears idle.
__global__ __launch_bounds__(RV_THREADS) void revive_count_kernel(const int32_t* __restrict__ idle, int GK, int revive_after,
                                                                  ReviveCounter* __restrict__ counter) {
    __shared__ unsigned wave_part[RV_WAVES];
    unsigned n = 0;
    for (int c = threadIdx.x; c < GK; c += RV_THREADS) n += idle[c] >= revive_after ? 1u : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) n += __shfl_xor(n, o, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) wave_part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < RV_WAVES; ++w) s += wave_part[w];
        counter->last = s;
        counter->total += s;
    }
}

// one wave per code.  VEC: D % 4 == 0 and every pointer 16-byte aligned
template <bool VEC>
__global__ __launch_bounds__(RV_THREADS) void revive_apply_kernel(const float* __restrict__ rows, int K, int D, int GK, int revive_after,
                                                                  int32_t* __restrict__ idle, float* __restrict__ E, float* __restrict__ m,
                                                                  float* __restrict__ v, float* __restrict__ vmax, float* __restrict__ ema_n,
                                                                  float* __restrict__ ema_m) {
    const int c = blockIdx.x * RV_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & (WAVE - 1);
    if (c >= GK) return;
    if (idle[c] < revive_after) return;                                  // not dead: not touched at all
    const size_t o = (size_t)c * D;
    if (VEC) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        for (int d = lane * 4; d < D; d += WAVE * 4) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(rows + o + d);
            *reinterpret_cast<f32x4*>(E + o + d) = x;
            if (m) *reinterpret_cast<f32x4*>(m + o + d) = zero;
            if (v) *reinterpret_cast<f32x4*>(v + o + d) = zero;
            if (vmax) *reinterpret_cast<f32x4*>(vmax + o + d) = zero;
            if (ema_m) *reinterpret_cast<f32x4*>(ema_m + o + d) = x;
        }
    } else {
        for (int d = lane; d < D; d += WAVE) {
            const float x = rows[o + d];
            E[o + d] = x;
            if (m) m[o + d] = 0.f;
            if (v) v[o + d] = 0.f;
            if (vmax) vmax[o + d] = 0.f;
            if (ema_m) ema_m[o + d] = x;
        }
    }
    if (lane == 0) {                                                     // (every lane has read idle[c] above: same wave, program order)
        if (ema_n) ema_n[c] = 1.0f;
        idle[c] = 0;
    }
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace kvq

using namespace kvq;

extern "C" {

int kvq_vq_usage_flags(const int64_t* idx, int64_t N, int K, int G, int32_t* used, void* stream) {
    KVQ_REQUIRE(idx && used, "kvq_vq_usage_flags: null pointer argument");
    KVQ_REQUIRE(N >= 1 && K >= 1 && G >= 1, "kvq_vq_usage_flags: N, K and G must be >= 1 (N=%lld K=%d G=%d)", (long long)N, K, G);
    KVQ_REQUIRE(N < (1ll << 32), "kvq_vq_usage_flags: N must be below 2^32, got %lld", (long long)N);
    KVQ_REQUIRE((long long)G * K <= INT32_MAX && G <= 65535, "kvq_vq_usage_flags: G * K must be below 2^31 and G below 65536 (K=%d G=%d)", K, G);
    KVQ_REQUIRE(((uintptr_t)idx & 7) == 0 && ((uintptr_t)used & 3) == 0, "kvq_vq_usage_flags: idx must be 8-byte and used 4-byte aligned");
    hipLaunchKernelGGL(usage_flags_kernel, dim3((K + RV_SLICE - 1) / RV_SLICE, G), dim3(RV_THREADS), 0, (hipStream_t)stream, idx,
                       (long long)N, K, used);
    return check_launch("usage_flags_kernel");
}

int kvq_vq_revive_select(const void* z, const int32_t* used, int64_t N, int K, int D, int G, int io_dtype, int revive_after,
                         uint64_t seed, int rank, int world, int32_t* idle, float* rows, void* stream) {
    KVQ_REQUIRE(z && used && idle && rows, "kvq_vq_revive_select: null pointer argument");
    KVQ_REQUIRE(N >= 1 && K >= 1 && D >= 1 && G >= 1, "kvq_vq_revive_select: N, K, D and G must be >= 1 (N=%lld K=%d D=%d G=%d)",
                (long long)N, K, D, G);
    KVQ_REQUIRE(N < (1ll << 32), "kvq_vq_revive_select: N must be below 2^32, got %lld", (long long)N);
    KVQ_REQUIRE((long long)G * K <= INT32_MAX, "kvq_vq_revive_select: G * K must be below 2^31 (K=%d G=%d)", K, G);
    KVQ_REQUIRE(revive_after >= 1, "kvq_vq_revive_select: revive_after must be >= 1, got %d", revive_after);
    KVQ_REQUIRE(world >= 1, "kvq_vq_revive_select: world must be >= 1, got %d", world);
    KVQ_REQUIRE(rank >= 0 && rank < world, "kvq_vq_revive_select: rank %d outside [0, world = %d)", rank, world);
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "kvq_vq_revive_select: unsupported io dtype %d", io_dtype);
    KVQ_REQUIRE(aligned16(z) && aligned16(rows), "kvq_vq_revive_select: 16-byte aligned z and rows required");
    KVQ_REQUIRE(((uintptr_t)used & 3) == 0 && ((uintptr_t)idle & 3) == 0, "kvq_vq_revive_select: 4-byte aligned used and idle required");
    const int GK = G * K;
    const dim3 grid((GK + RV_WAVES - 1) / RV_WAVES), block(RV_THREADS);
    hipStream_t st = (hipStream_t)stream;
    const unsigned long long* off = seed_offset_ptr();
#define RV_SELECT(DT, VEC)                                                                                                            \
    hipLaunchKernelGGL((revive_select_kernel<DT, VEC>), grid, block, 0, st, z, used, (long long)N, K, D, GK, revive_after,            \
                       (unsigned long long)seed, off, rank, world, idle, rows)
    if (io_dtype == KVQ_F32) {
        if (D % 4 == 0) RV_SELECT(KVQ_F32, true); else RV_SELECT(KVQ_F32, false);
    } else {
        if (D % 8 == 0) RV_SELECT(KVQ_BF16, true); else RV_SELECT(KVQ_BF16, false);
    }
#undef RV_SELECT
    return check_launch("revive_select_kernel");
}

int kvq_vq_revive_apply(const float* rows, int K, int D, int G, int revive_after, int32_t* idle, float* E, float* m, float* v,
                        float* vmax, float* ema_n, float* ema_m, void* counter, void* stream) {
    KVQ_REQUIRE(rows && idle && E && counter, "kvq_vq_revive_apply: null pointer argument");
    KVQ_REQUIRE(K >= 1 && D >= 1 && G >= 1, "kvq_vq_revive_apply: K, D and G must be >= 1 (K=%d D=%d G=%d)", K, D, G);
    KVQ_REQUIRE((long long)G * K <= INT32_MAX, "kvq_vq_revive_apply: G * K must be below 2^31 (K=%d G=%d)", K, G);
    KVQ_REQUIRE(revive_after >= 1, "kvq_vq_revive_apply: revive_after must be >= 1, got %d", revive_after);
    KVQ_REQUIRE(aligned16(rows) && aligned16(E), "kvq_vq_revive_apply: 16-byte aligned rows and E required");
    KVQ_REQUIRE(((uintptr_t)idle & 3) == 0 && ((uintptr_t)counter & 7) == 0 && ((uintptr_t)m & 3) == 0 && ((uintptr_t)v & 3) == 0 &&
                    ((uintptr_t)vmax & 3) == 0 && ((uintptr_t)ema_n & 3) == 0 && ((uintptr_t)ema_m & 3) == 0,
                "kvq_vq_revive_apply: 4-byte aligned idle and moments, 8-byte aligned counter required");
    const int GK = G * K;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(revive_count_kernel, dim3(1), dim3(RV_THREADS), 0, st, idle, GK, revive_after, (ReviveCounter*)counter);
    int rc = check_launch("revive_count_kernel");
    if (rc) return rc;
    const dim3 grid((GK + RV_WAVES - 1) / RV_WAVES), block(RV_THREADS);
    const bool vec = D % 4 == 0 && aligned16(m) && aligned16(v) && aligned16(vmax) && aligned16(ema_m);
    if (vec)
        hipLaunchKernelGGL(revive_apply_kernel<true>, grid, block, 0, st, rows, K, D, GK, revive_after, idle, E, m, v, vmax, ema_n, ema_m);
    else
        hipLaunchKernelGGL(revive_apply_kernel<false>, grid, block, 0, st, rows, K, D, GK, revive_after, idle, E, m, v, vmax, ema_n, ema_m);
    return check_launch("revive_apply_kernel");
}

}  // extern "C"
