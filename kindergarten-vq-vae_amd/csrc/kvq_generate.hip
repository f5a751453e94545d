// kvq_generate.hip -- free-running generation: one decoder token per sentence and launch, over a key/value cache (gfx950).
//
// TrainEngine.generate runs the decoder one position at a time: [B, H] rows through the GEMMs the training step uses, and the
// kernels of this file for what is not a GEMM or a LayerNorm:
//     kvq_gen_embed     BertEmbeddings of the token at column t of `ids` (the bits of kvq_embed_ln_fwd's row for it)
//     kvq_gen_attn      one query row per (sentence, head) against the cache (self-attention: this step's k | v rows are appended
//                       first) or against the projected latent (cross-attention)
//     kvq_gen_select    the next token: arg-max of logit / tau + Gumbel noise (none when greedy), prompt / end-token bookkeeping
//     kvq_gen_select_filtered   the same from a top-k / top-p filtered distribution, with the score of the choice (filter state)
//     kvq_gen_advance   one thread: t += 1
// Every kernel reads the position t from the 32-byte generation state on the device (include/kvq.h), so one captured chain of
// launches serves every position.  No atomics, fixed summation orders: the same inputs give the same bits.
//
// kvq_gen_attn is a read of K and V, at most 128 rows of 64 elements per (sentence, head): 16 bytes per lane straight to
// registers (8 lanes span a bf16 row, 16 an f32 row; a wave takes 8 resp. 4 keys per instruction, four instructions in flight),
// no LDS staging of the operands and no MFMA -- a single query row would fill one row of a 32 x 32 tile.  The scores pass through
// 512 bytes of LDS between the three phases (scores, softmax, P.V).
#include <math.h>

#include "kvq_common.h"
#include <type_traits>

namespace kvq {

struct GenState {
    int32_t t, P, Lmax, eos_id, pad_id;
    uint32_t seed_lo, seed_hi;      // the Philox key of the sampling draws
    float inv_tau;                  // 1 / temperature; 0 = greedy (no noise, the logits as they are)
};
static_assert(sizeof(GenState) == 32, "the generation state is 32 bytes (include/kvq.h)");

constexpr int GEN_MAX_KEYS = 128;
constexpr int GEN_LN_MAX_PER_LANE = 16;   // H <= 4096, as csrc/kvq_ln.hip

__device__ __forceinline__ float gen_wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, WAVE));
    return v;
}

// ---------------------------------------------------------------------------------------------------------------
// embedding: embed_ln_fwd_kernel of csrc/kvq_ln.hip for the rows (b, t), restated operation by operation (p_drop = 0): one wave
// per row, lane `lane` holds the chunks lane + 64 u of 4 elements, the sums in that kernel's order
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gen_quadsum(f32x4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float gen_dot4(f32x4 a, f32x4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }

template <int DT, int PER>
__global__ __launch_bounds__(256) void gen_embed_kernel(const GenState* __restrict__ st, const int64_t* __restrict__ ids,
                                                         const void* __restrict__ word, const void* __restrict__ pos,
                                                         const void* __restrict__ type_row, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, int B, int H, int64_t V, int pos_rows,
                                                         float eps, void* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const int t = st->t, Lmax = st->Lmax;
    if (t < 0 || t >= Lmax || t >= pos_rows) return;          // (uniform) a state outside the buffers: nothing is read or stored
    const int nchunk = H >> 2;
    int64_t id = ids[(int64_t)row * Lmax + t];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);
    f32x4 v[PER];
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int c = lane + WAVE * u;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (c < nchunk) {
            f32x4 pt = IO<DT>::load4(pos, (size_t)t * H + 4 * c) + IO<DT>::load4(type_row, 4 * c);
            pt.x = IO<DT>::round(pt.x); pt.y = IO<DT>::round(pt.y); pt.z = IO<DT>::round(pt.z); pt.w = IO<DT>::round(pt.w);
            a = IO<DT>::load4(word, (size_t)id * H + 4 * c) + pt;
            a.x = IO<DT>::round(a.x); a.y = IO<DT>::round(a.y); a.z = IO<DT>::round(a.z); a.w = IO<DT>::round(a.w);
            sum += gen_quadsum(a);
        }
        v[u] = a;
    }
    const float mean = wave_sum_f32(sum) / (float)H;
    float sq = 0.f;
#pragma unroll
    for (int u = 0; u < PER; ++u)
        if (lane + WAVE * u < nchunk) {
            const f32x4 d = v[u] - mean;
            sq += gen_dot4(d, d);
        }
    const float var = wave_sum_f32(sq) / (float)H;
    const float rstd = rsqrtf(var + eps);
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int c = lane + WAVE * u;
        if (c < nchunk) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * c);
            const f32x4 b = *reinterpret_cast<const f32x4*>(beta + 4 * c);
            const f32x4 o = (v[u] - mean) * rstd * g + b;
            IO<DT>::store4(out, (size_t)row * H + 4 * c, o);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// attention of one query row.  One wave per (sentence, head).  EPL elements (16 bytes) per lane, LPR lanes per 64-element row,
// KPI rows per wave instruction, GEN_UNROLL instructions in flight.
// ---------------------------------------------------------------------------------------------------------------
constexpr int GEN_UNROLL = 4;

template <int DT>
struct Chunk;
template <>
struct Chunk<KVQ_BF16> {
    static constexpr int EPL = 8;
    typedef uint4 raw;
    __device__ static __forceinline__ void unpack(const raw& r, float (&f)[8]) {
        f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
        f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
        f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
        f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
    }
    __device__ static __forceinline__ raw pack(const float (&f)[8]) {
        raw r;
        r.x = (unsigned)f32_to_bf16(f[0]) | ((unsigned)f32_to_bf16(f[1]) << 16);
        r.y = (unsigned)f32_to_bf16(f[2]) | ((unsigned)f32_to_bf16(f[3]) << 16);
        r.z = (unsigned)f32_to_bf16(f[4]) | ((unsigned)f32_to_bf16(f[5]) << 16);
        r.w = (unsigned)f32_to_bf16(f[6]) | ((unsigned)f32_to_bf16(f[7]) << 16);
        return r;
    }
};
template <>
struct Chunk<KVQ_F32> {
    static constexpr int EPL = 4;
    typedef f32x4 raw;
    __device__ static __forceinline__ void unpack(const raw& r, float (&f)[4]) { f[0] = r.x; f[1] = r.y; f[2] = r.z; f[3] = r.w; }
    __device__ static __forceinline__ raw pack(const float (&f)[4]) {
        raw r = {f[0], f[1], f[2], f[3]};
        return r;
    }
};

// BEAM (kvq_beam_attn): the same arithmetic, lane mapping and summation order with two indirections in the ADDRESSES.  Self-attention:
// key j < t of row b is row j of the cache of slot anc[t & 1][b, j] (the ancestry table of beam search, [2, B, anc_ld] int32; the row
// is staged in LDS once); the step's own rows still go to row (b, t).  Cross-attention: row b reads sentence b / rows_per_sentence.
template <int DT, bool BEAM>
__device__ __forceinline__ void gen_attn_body(const GenState* __restrict__ st, const void* __restrict__ q, int64_t ldq,
                                              const void* __restrict__ k_new, const void* __restrict__ v_new, int64_t ld_new, void* kv,
                                              int64_t ld_kv, int64_t kv_sentence_stride, int nh, int append, int n_keys, int Smax,
                                              void* __restrict__ out, int64_t ldo, const int32_t* __restrict__ anc, int64_t anc_half,
                                              int anc_ld, int rows_per_sentence, int n_rows) {
    typedef typename IO<DT>::elem elem;
    typedef Chunk<DT> CH;
    typedef typename CH::raw raw;
    constexpr int EPL = CH::EPL, LPR = 64 / EPL, KPI = WAVE / LPR;
    __shared__ float sc[GEN_MAX_KEYS];
    __shared__ int slot[BEAM ? GEN_MAX_KEYS : 1];

    const int b = blockIdx.x / nh, h = blockIdx.x - b * nh;
    const int lane = threadIdx.x, sub = lane % LPR, grp = lane / LPR;
    const int t = st->t;
    if (append && (t < 0 || t >= Smax)) return;               // (uniform) no row t in the cache: nothing is read or stored
    const int n = append ? t + 1 : n_keys;                    // 1 .. 128
    const int col = h * 64 + sub * EPL;

    const int src = BEAM && !append ? b / rows_per_sentence : b;     // the sentence whose keys this row reads (cross-attention)
    const elem* kbase = reinterpret_cast<const elem*>(kv) + (size_t)src * kv_sentence_stride + col;
    const elem* vbase = kbase + (size_t)nh * 64;
    if constexpr (BEAM) {
        if (append) {                                         // (uniform) the slots of keys 0 .. t; a slot outside the cache reads row b
            const int32_t* arow = anc + (size_t)(t & 1) * anc_half + (size_t)b * anc_ld;
            for (int j = lane; j < n; j += WAVE) {
                const int s = arow[j];
                slot[j] = s >= 0 && s < n_rows ? s : b;
            }
            __syncthreads();
        }
    }
    // row j of the keys (of the values: + nh * 64) as this query reads it
    auto key_row = [&](int j) -> const elem* {
        if constexpr (BEAM) {
            if (append) return reinterpret_cast<const elem*>(kv) + (size_t)slot[j] * kv_sentence_stride + (size_t)j * ld_kv + col;
        }
        return kbase + (size_t)j * ld_kv;
    };
    const elem* knew = append ? reinterpret_cast<const elem*>(k_new) + (size_t)b * ld_new + col : kbase;
    const elem* vnew = append ? reinterpret_cast<const elem*>(v_new) + (size_t)b * ld_new + col : vbase;
    const int fresh = append ? t : -1;                        // the key whose row comes from this step's projection, not from the cache

    float qf[EPL];
    CH::unpack(*reinterpret_cast<const raw*>(reinterpret_cast<const elem*>(q) + (size_t)b * ldq + col), qf);

    if (append && grp < 2) {                                  // this step's k (group 0) and v (group 1) rows go to row t of the cache
        const raw r = *reinterpret_cast<const raw*>(grp == 0 ? knew : vnew);
        elem* dst = reinterpret_cast<elem*>(kv) + (size_t)b * kv_sentence_stride + (size_t)t * ld_kv + col + (grp == 0 ? 0 : nh * 64);
        *reinterpret_cast<raw*>(dst) = r;
    }

    // ---- scores: s_j = (q . k_j) / 8 ----
    for (int j0 = 0; j0 < n; j0 += KPI * GEN_UNROLL) {
        raw r[GEN_UNROLL];
#pragma unroll
        for (int u = 0; u < GEN_UNROLL; ++u) {
            const int j = j0 + u * KPI + grp;
            const int jc = j < n ? j : n - 1;                 // (rows past the last key: a valid row, the score is not stored)
            r[u] = *reinterpret_cast<const raw*>(jc == fresh ? knew : key_row(jc));
        }
#pragma unroll
        for (int u = 0; u < GEN_UNROLL; ++u) {
            const int j = j0 + u * KPI + grp;
            float kf[EPL];
            CH::unpack(r[u], kf);
            float d = 0.f;
#pragma unroll
            for (int e = 0; e < EPL; ++e) d += qf[e] * kf[e];
#pragma unroll
            for (int m = LPR / 2; m >= 1; m >>= 1) d += __shfl_xor(d, m, WAVE);
            if (sub == 0 && j < n) sc[j] = d * 0.125f;
        }
    }
    __syncthreads();

    // ---- softmax over the n scores, f32; the probabilities stay unnormalised until the output ----
    const float s0 = lane < n ? sc[lane] : -INFINITY, s1 = lane + 64 < n ? sc[lane + 64] : -INFINITY;
    const float mx = gen_wave_max(fmaxf(s0, s1));
    const float p0 = lane < n ? __expf(s0 - mx) : 0.f, p1 = lane + 64 < n ? __expf(s1 - mx) : 0.f;
    const float inv = 1.0f / wave_sum_f32(p0 + p1);
    __syncthreads();
    if (lane < n) sc[lane] = p0;
    if (lane + 64 < n) sc[lane + 64] = p1;
    __syncthreads();

    // ---- out = (sum_j p_j v_j) / sum_j p_j : each lane group adds its keys in ascending order, then the groups are added ----
    float acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    for (int j0 = 0; j0 < n; j0 += KPI * GEN_UNROLL) {
        raw r[GEN_UNROLL];
        float p[GEN_UNROLL];
#pragma unroll
        for (int u = 0; u < GEN_UNROLL; ++u) {
            const int j = j0 + u * KPI + grp;
            const int jc = j < n ? j : n - 1;
            r[u] = *reinterpret_cast<const raw*>(jc == fresh ? vnew : key_row(jc) + (size_t)nh * 64);
            p[u] = j < n ? sc[jc] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < GEN_UNROLL; ++u) {
            float vf[EPL];
            CH::unpack(r[u], vf);
#pragma unroll
            for (int e = 0; e < EPL; ++e) acc[e] += p[u] * vf[e];
        }
    }
#pragma unroll
    for (int m = LPR; m < WAVE; m <<= 1)
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] += __shfl_xor(acc[e], m, WAVE);
    if (grp == 0) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] *= inv;
        *reinterpret_cast<raw*>(reinterpret_cast<elem*>(out) + (size_t)b * ldo + col) = CH::pack(acc);
    }
}

template <int DT>
__global__ __launch_bounds__(64) void gen_attn_kernel(const GenState* __restrict__ st, const void* __restrict__ q, int64_t ldq,
                                                       const void* __restrict__ k_new, const void* __restrict__ v_new, int64_t ld_new,
                                                       void* kv, int64_t ld_kv, int64_t kv_sentence_stride, int nh, int append,
                                                       int n_keys, int Smax, void* __restrict__ out, int64_t ldo) {
    gen_attn_body<DT, false>(st, q, ldq, k_new, v_new, ld_new, kv, ld_kv, kv_sentence_stride, nh, append, n_keys, Smax, out, ldo, nullptr, 0, 0, 1, 0);
}

template <int DT>
__global__ __launch_bounds__(64) void beam_attn_kernel(const GenState* __restrict__ st, const void* __restrict__ q, int64_t ldq,
                                                        const void* __restrict__ k_new, const void* __restrict__ v_new, int64_t ld_new,
                                                        void* kv, int64_t ld_kv, int64_t kv_sentence_stride, int nh, int append,
                                                        int n_keys, int Smax, void* __restrict__ out, int64_t ldo,
                                                        const int32_t* __restrict__ anc, int64_t anc_half, int anc_ld, int rows_per_sentence,
                                                        int n_rows) {
    gen_attn_body<DT, true>(st, q, ldq, k_new, v_new, ld_new, kv, ld_kv, kv_sentence_stride, nh, append, n_keys, Smax, out, ldo, anc, anc_half,
                            anc_ld, rows_per_sentence, n_rows);
}

// ---------------------------------------------------------------------------------------------------------------
// next token: one workgroup of 256 threads per sentence
// ---------------------------------------------------------------------------------------------------------------
constexpr int SEL_THREADS = 256;

// Gumbel(0, 1) from 32 random bits, FINITE for every bit pattern: u = (k + 1/2) 2^-23 with the 23-bit k = b >> 9 is exact in f32
// (k + 1/2 needs 24 significant bits) and lies in [2^-24, 1 - 2^-24]; logf (not the fast form, whose absolute error near 1 could
// round -log u to 0) gives -log u in [5.96e-8, 16.7], so g lies in [-2.82, 16.7].  (With 24 bits, (k + 1/2) rounds to 2^24 for
// k = 2^24 - 1: u = 1, g = +inf, and that column would win whatever its logit -- once in 550 tokens of a 30522-word vocabulary.)
__device__ __forceinline__ float gen_gumbel_from_bits(unsigned b) {
    const float u = ((float)(b >> 9) + 0.5f) * (1.0f / 8388608.0f);
    return -logf(-logf(u));
}
// strictly larger wins, equal -> lower index; a NaN compares false both ways and never wins
__device__ __forceinline__ bool sel_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

template <int DT>
__global__ __launch_bounds__(SEL_THREADS) void gen_select_kernel(const GenState* __restrict__ st, const void* __restrict__ logits,
                                                                  int64_t ld, int V, int64_t* __restrict__ ids, int32_t* __restrict__ finished,
                                                                  int32_t* __restrict__ lengths, float* __restrict__ step_logits) {
    __shared__ float wv[SEL_THREADS / WAVE];
    __shared__ int wi[SEL_THREADS / WAVE];
    const int b = blockIdx.x;
    const int t = st->t, Lmax = st->Lmax;
    if (t < 0 || t >= Lmax) return;                           // (uniform)
    const bool sample = st->inv_tau > 0.f;                    // (uniform) temperature and seed come from the state, as t does: one
    const float inv_tau = sample ? st->inv_tau : 1.0f;        // captured step serves every seed and temperature
    const unsigned k0 = st->seed_lo, k1 = st->seed_hi;
    float* lrow = step_logits ? step_logits + ((size_t)b * Lmax + t) * V : nullptr;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    const int nchunk = (V + 7) >> 3;                          // 8 columns at a time (ld % 8 == 0: the chunk lies inside the row)
    for (int c = threadIdx.x; c < nchunk; c += SEL_THREADS) {
        const f32x8 x8 = IO<DT>::load8(logits, (size_t)b * ld + 8 * c);
        const float x[8] = {x8.lo.x, x8.lo.y, x8.lo.z, x8.lo.w, x8.hi.x, x8.hi.y, x8.hi.z, x8.hi.w};
        float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (sample) {                                         // (uniform)
            const U4 r0 = philox4x32((unsigned)(2 * c), (unsigned)b, (unsigned)t, 0x47454e53u, k0, k1);
            const U4 r1 = philox4x32((unsigned)(2 * c + 1), (unsigned)b, (unsigned)t, 0x47454e53u, k0, k1);
            g[0] = gen_gumbel_from_bits(r0.x); g[1] = gen_gumbel_from_bits(r0.y); g[2] = gen_gumbel_from_bits(r0.z); g[3] = gen_gumbel_from_bits(r0.w);
            g[4] = gen_gumbel_from_bits(r1.x); g[5] = gen_gumbel_from_bits(r1.y); g[6] = gen_gumbel_from_bits(r1.z); g[7] = gen_gumbel_from_bits(r1.w);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int v = 8 * c + e;
            if (v < V) {
                if (lrow) lrow[v] = x[e];
                const float s = x[e] * inv_tau + g[e];
                if (sel_better(s, v, bv, bi)) { bv = s; bi = v; }
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(bv, m, WAVE);
        const int oi = __shfl_xor(bi, m, WAVE);
        if (sel_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { wv[threadIdx.x >> 6] = bv; wi[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < SEL_THREADS / WAVE; ++w)
            if (sel_better(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
        const int choice = bi == 0x7fffffff ? 0 : bi;          // (a row of NaNs)
        if (t + 1 < Lmax && t + 1 >= st->P) {                  // (inside the prompt the token that is there is kept)
            int64_t* dst = ids + (size_t)b * Lmax + t + 1;
            if (finished[b]) {
                *dst = st->pad_id;
            } else {
                *dst = choice;
                if (choice == st->eos_id) { finished[b] = 1; lengths[b] = t + 2; }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// next token from a top-k / top-p filtered distribution (include/kvq.h "kvq_gen_select_filtered"): one workgroup of 1024 threads
// per sentence, the row read ONCE, 16 bytes a lane, and kept in registers (FLT_CHUNKS chunks of 8 columns a thread: V <= 32768).
//
// The kept set is a prefix of the order (y descending, then the index ascending), so it is known by its LAST element: a threshold
// value and, inside the group tied at it, an index.  Both are selections, found bit by bit: y maps to an order-preserving 32-bit
// key (0 = a NaN or a column >= V), and a round asks "does the cut lie among the keys that continue the decided prefix with a 1?"
// from ONE block reduction of their count (top-k) and of their mass (top-p) -- rank and mass above a threshold are both monotone
// in it.  Members of the tied group share one mass, so the number of them to keep follows from the count or the mass that is left,
// and the index of the last of them is a second, 16-bit, selection.  top-k before top-p: the first search gives Z of the top k.
//
// Summation order of every mass (the premise of TOL_MASS, include/kvq.h): a thread adds its chunk of 8 as a tree (3 roundings),
// its chunks in ascending order (3), the wave is a butterfly (6), the 16 waves a tree (4): 16 roundings; the mass above the
// threshold is the sum of at most 32 such round sums in the order of the rounds (32), then + j e_T (2).  Every thread forms the
// same sums from the same LDS words, so every decision is uniform; no atomics.
// ---------------------------------------------------------------------------------------------------------------
struct GenFilter {
    int32_t top_k;                  // <= 0: off
    float top_p;                    // outside (0, 1): off
    int32_t reserved[2];            // 0; anything else: the kernel stores nothing
};
static_assert(sizeof(GenFilter) == 16, "the filter state is 16 bytes (include/kvq.h)");

constexpr int FLT_THREADS = 1024;
constexpr int FLT_WAVES = FLT_THREADS / WAVE;
constexpr int FLT_CHUNKS = 4;
constexpr int FLT_N = FLT_CHUNKS * 8;                       // columns a thread holds
constexpr int FLT_MAX_V = FLT_THREADS * FLT_N;              // 32768
static_assert(FLT_WAVES == 16, "the wave tree of flt_reduce is written for 16 waves");

// y -> key: larger y, larger key; -0 counts as +0 (they compare equal); a NaN -> 0, below every value (-inf -> 0x007fffff)
__device__ __forceinline__ unsigned flt_key(float y) {
    if (y != y) return 0u;
    const unsigned u = __float_as_uint(y == 0.f ? 0.f : y);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float flt_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

struct FltShared {
    int c[2][FLT_WAVES];            // two slots, used in turn: one barrier a reduction
    float m[2][FLT_WAVES];
    float av[FLT_WAVES], ay[FLT_WAVES];
    int ai[FLT_WAVES];
};

__device__ __forceinline__ float flt_tree8(const float (&a)[8]) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])); }

// (c, m) of the thread -> of the workgroup, the same bits in every thread.  MODE 0: c only; 1: c and the sum of m; 2: c and the max of m
template <int MODE>
__device__ __forceinline__ void flt_reduce(int& c, float& m, FltShared& sh, int& slot, int lane, int wave) {
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        c += __shfl_xor(c, k, WAVE);
        if (MODE == 1) m += __shfl_xor(m, k, WAVE);
        if (MODE == 2) m = fmaxf(m, __shfl_xor(m, k, WAVE));
    }
    if (lane == 0) {
        sh.c[slot][wave] = c;
        if (MODE != 0) sh.m[slot][wave] = m;
    }
    __syncthreads();
    int cc[FLT_WAVES];
    float mm[FLT_WAVES];
#pragma unroll
    for (int w = 0; w < FLT_WAVES; ++w) {
        cc[w] = sh.c[slot][w];
        mm[w] = MODE != 0 ? sh.m[slot][w] : 0.f;
    }
#pragma unroll
    for (int s = 1; s < FLT_WAVES; s <<= 1)
#pragma unroll
        for (int w = 0; w < FLT_WAVES; w += 2 * s) {
            cc[w] += cc[w + s];
            if (MODE == 1) mm[w] += mm[w + s];
            if (MODE == 2) mm[w] = fmaxf(mm[w], mm[w + s]);
        }
    c = cc[0];
    m = mm[0];
    slot ^= 1;
}

// The last element of the order by `key` (descending) that is kept: T = its key, cnt_gt / mass_gt = count and mass of the keys
// above T.  Kept is what comes before the count reaches kk (1 <= kk <= the keys that are not 0) or, with MASS, before the mass
// reaches `target`, whichever is first.  Bits top_bit .. 0, the key's upper bits are 0.  kk comes back lowered to the end of the
// last half the search entered, so that ca < kk <= ca + (keys left) holds in every round and T is the key of an element.
template <bool MASS>
__device__ __forceinline__ void flt_search(const unsigned (&key)[FLT_N], const float (&e)[FLT_N], int top_bit, int& kk, float target,
                                           FltShared& sh, int& slot, int lane, int wave, unsigned& T, int& cnt_gt, float& mass_gt) {
    unsigned prefix = 0;
    int ca = 0;
    float ma = 0.f;
    for (int bit = top_bit; bit >= 0; --bit) {
        const unsigned cand = (prefix >> bit) | 1u;            // the upper half of what is left: bits 31 .. bit equal to cand
        int c = 0;
        float m = 0.f;
#pragma unroll
        for (int u = 0; u < FLT_CHUNKS; ++u) {
            float a[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const bool hit = (key[8 * u + i] >> bit) == cand;
                c += hit ? 1 : 0;
                a[i] = MASS && hit ? e[8 * u + i] : 0.f;
            }
            if (MASS) m += flt_tree8(a);
        }
        flt_reduce<MASS ? 1 : 0>(c, m, sh, slot, lane, wave);
        const bool up = ca + c >= kk || (MASS && c > 0 && ma + m >= target);
        if (up) {
            prefix |= 1u << bit;
            kk = min(kk, ca + c);                              // the cut lies in this half at the latest at its end -- also when the mass,
        } else {                                               // summed again in finer pieces, falls short of the target by a rounding
            ca += c;
            if (MASS) ma = ma + m;
        }
    }
    T = prefix;
    cnt_gt = ca;
    mass_gt = ma;
}

// The cut in full: T as flt_search, j = how many of the ntie keys equal to T are kept (by index order), n_keep = cnt_gt + j,
// C = mass_gt + j e_T, the mass of the kept set.
template <bool MASS>
__device__ __forceinline__ void flt_cut(const unsigned (&key)[FLT_N], const float (&e)[FLT_N], int kk, float target, float mx, FltShared& sh,
                                        int& slot, int lane, int wave, unsigned& T, int& j, int& n_keep, float& C) {
    int cg;
    float mg;
    flt_search<MASS>(key, e, 31, kk, target, sh, slot, lane, wave, T, cg, mg);
    int ntie = 0;
    float above = 0.f;
#pragma unroll
    for (int u = 0; u < FLT_CHUNKS; ++u) {
        float a[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            ntie += key[8 * u + i] == T ? 1 : 0;
            a[i] = !MASS && key[8 * u + i] > T ? e[8 * u + i] : 0.f;
        }
        if (!MASS) above += flt_tree8(a);
    }
    flt_reduce<1>(ntie, above, sh, slot, lane, wave);
    if (!MASS) mg = above;
    const float eT = expf(flt_unkey(T) - mx);                  // the bits every member of the group holds
    const int jk = min(kk - cg, ntie);
    int jp = ntie;
    if (MASS) {                                                // the smallest j in 1 .. ntie with mass_gt + j e_T >= target, else ntie
        int lo = 1, hi = ntie;
        if (mg + (float)hi * eT >= target) {
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (mg + (float)mid * eT >= target) hi = mid;
                else lo = mid + 1;
            }
            jp = lo;
        }
    }
    j = min(jk, jp);
    n_keep = cg + j;
    C = mg + (float)j * eT;
}

template <int DT>
__global__ __launch_bounds__(FLT_THREADS) void gen_select_filtered_kernel(const GenState* __restrict__ st, const GenFilter* __restrict__ fs,
                                                                           const void* __restrict__ logits, int64_t ld, int V,
                                                                           int64_t* __restrict__ ids, int32_t* __restrict__ finished,
                                                                           int32_t* __restrict__ lengths, float* __restrict__ step_logits,
                                                                           int32_t* __restrict__ step_kept, int32_t* __restrict__ step_cut,
                                                                           float* __restrict__ step_logprob) {
    __shared__ FltShared sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = st->t, Lmax = st->Lmax;
    if (t < 0 || t >= Lmax) return;                            // (uniform)
    if (fs->reserved[0] != 0 || fs->reserved[1] != 0) return;  // (uniform) a filter state this kernel does not know
    const bool sample = st->inv_tau > 0.f;                     // (uniform)
    const float inv_tau = sample ? st->inv_tau : 1.0f;
    const unsigned k0 = st->seed_lo, k1 = st->seed_hi;
    const int top_k = fs->top_k;
    const float top_p = fs->top_p;
    float* lrow = step_logits ? step_logits + ((size_t)b * Lmax + t) * V : nullptr;
    const size_t at = (size_t)b * Lmax + t;
    int slot = 0;

    // ---- the row: keys, the count of valid columns, the maximum ----
    unsigned key[FLT_N];
    float e[FLT_N];                                            // y first, exp(y - max) then
    const int nchunk = (V + 7) >> 3;                           // (ld % 8 == 0: the chunk lies inside the row)
    int nv = 0;
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < FLT_CHUNKS; ++u) {
        const int c = tid + FLT_THREADS * u;
        if (c < nchunk) {
            const f32x8 x8 = IO<DT>::load8(logits, (size_t)b * ld + 8 * c);
            const float x[8] = {x8.lo.x, x8.lo.y, x8.lo.z, x8.lo.w, x8.hi.x, x8.hi.y, x8.hi.z, x8.hi.w};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int v = 8 * c + i;
                unsigned k = 0u;
                float y = 0.f;
                if (v < V) {
                    if (lrow) lrow[v] = x[i];
                    y = x[i] * inv_tau;
                    k = flt_key(y);
                }
                key[8 * u + i] = k;
                e[8 * u + i] = y;
                if (k != 0u) { nv += 1; mx = fmaxf(mx, y); }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) { key[8 * u + i] = 0u; e[8 * u + i] = 0.f; }
        }
    }
    flt_reduce<2>(nv, mx, sh, slot, lane, wave);

    bool store = false;                                        // (uniform) whether column t + 1 takes the choice
    if (t + 1 < Lmax && t + 1 >= st->P) store = true;
    if (nv == 0) {                                             // (uniform) a row with no valid logit: 0, as kvq_gen_select
        if (tid == 0) {
            if (store) {
                int64_t* dst = ids + (size_t)b * Lmax + t + 1;
                if (finished[b]) {
                    *dst = st->pad_id;
                } else {
                    *dst = 0;
                    if (0 == st->eos_id) { finished[b] = 1; lengths[b] = t + 2; }
                }
            }
            if (step_kept) step_kept[at] = 0;
            if (step_cut) step_cut[at] = -1;
            if (step_logprob) step_logprob[at] = __builtin_nanf("");
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < FLT_N; ++i) e[i] = key[i] != 0u ? expf(e[i] - mx) : 0.f;

    // ---- the cut ----
    const bool need_k = sample && top_k >= 1 && top_k < nv;    // (uniform; a greedy state ignores the filters)
    const bool need_p = sample && top_p > 0.f && top_p < 1.f;
    const int kk = need_k ? top_k : nv;
    unsigned T;
    int j, n_keep;
    float C;
    if (need_p) {
        float Z;
        if (need_k) {                                          // Z of the first kk of the order
            flt_cut<false>(key, e, kk, INFINITY, mx, sh, slot, lane, wave, T, j, n_keep, Z);
        } else {
            int none = 0;
            Z = 0.f;
#pragma unroll
            for (int u = 0; u < FLT_CHUNKS; ++u) {
                const float a[8] = {e[8 * u], e[8 * u + 1], e[8 * u + 2], e[8 * u + 3], e[8 * u + 4], e[8 * u + 5], e[8 * u + 6], e[8 * u + 7]};
                Z += flt_tree8(a);
            }
            flt_reduce<1>(none, Z, sh, slot, lane, wave);
        }
        flt_cut<true>(key, e, kk, top_p * Z, mx, sh, slot, lane, wave, T, j, n_keep, C);
    } else {
        flt_cut<false>(key, e, kk, INFINITY, mx, sh, slot, lane, wave, T, j, n_keep, C);
    }

    // ---- the index of the j-th (by index) of the group tied at T ----
    unsigned k2[FLT_N];
#pragma unroll
    for (int u = 0; u < FLT_CHUNKS; ++u)
#pragma unroll
        for (int i = 0; i < 8; ++i) k2[8 * u + i] = key[8 * u + i] == T ? (unsigned)(FLT_MAX_V - (8 * (tid + FLT_THREADS * u) + i)) : 0u;
    unsigned T2;
    int cg2;
    float mg2;
    int j2 = j;
    flt_search<false>(k2, e, 15, j2, INFINITY, sh, slot, lane, wave, T2, cg2, mg2);
    const int cut = FLT_MAX_V - (int)T2;

    // ---- the choice: first arg-max of y + g over the kept set, g as kvq_gen_select draws it ----
    float bv = -INFINITY, by = 0.f;
    int bi = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < FLT_CHUNKS; ++u) {
        const int c = tid + FLT_THREADS * u;
        bool kept[8], any = false;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            kept[i] = key[8 * u + i] > T || (key[8 * u + i] == T && 8 * c + i <= cut);
            any |= kept[i];
        }
        if (any) {
            float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (sample) {                                      // (uniform)
                const U4 r0 = philox4x32((unsigned)(2 * c), (unsigned)b, (unsigned)t, 0x47454e53u, k0, k1);
                const U4 r1 = philox4x32((unsigned)(2 * c + 1), (unsigned)b, (unsigned)t, 0x47454e53u, k0, k1);
                g[0] = gen_gumbel_from_bits(r0.x); g[1] = gen_gumbel_from_bits(r0.y); g[2] = gen_gumbel_from_bits(r0.z); g[3] = gen_gumbel_from_bits(r0.w);
                g[4] = gen_gumbel_from_bits(r1.x); g[5] = gen_gumbel_from_bits(r1.y); g[6] = gen_gumbel_from_bits(r1.z); g[7] = gen_gumbel_from_bits(r1.w);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (kept[i]) {
                    const float y = flt_unkey(key[8 * u + i]);
                    const float s = y + g[i];
                    if (sel_better(s, 8 * c + i, bv, bi)) { bv = s; bi = 8 * c + i; by = y; }
                }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(bv, m, WAVE), oy = __shfl_xor(by, m, WAVE);
        const int oi = __shfl_xor(bi, m, WAVE);
        if (sel_better(ov, oi, bv, bi)) { bv = ov; bi = oi; by = oy; }
    }
    if (lane == 0) { sh.av[wave] = bv; sh.ai[wave] = bi; sh.ay[wave] = by; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < FLT_WAVES; ++w)
            if (sel_better(sh.av[w], sh.ai[w], bv, bi)) { bv = sh.av[w]; bi = sh.ai[w]; by = sh.ay[w]; }
        const int choice = bi == 0x7fffffff ? 0 : bi;
        if (store) {
            int64_t* dst = ids + (size_t)b * Lmax + t + 1;
            if (finished[b]) {
                *dst = st->pad_id;
            } else {
                *dst = choice;
                if (choice == st->eos_id) { finished[b] = 1; lengths[b] = t + 2; }
            }
        }
        if (step_kept) step_kept[at] = n_keep;
        if (step_cut) step_cut[at] = cut;
        if (step_logprob) step_logprob[at] = bi == 0x7fffffff ? __builtin_nanf("") : (by - mx) - logf(C);
    }
}

__global__ void gen_advance_kernel(GenState* st) { st->t += 1; }

__global__ void gen_gumbel_debug_kernel(const unsigned* __restrict__ bits, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = gen_gumbel_from_bits(bits[i]);
}

// ---------------------------------------------------------------------------------------------------------------
// beam search: one step of the search of one sentence per workgroup of 1024 threads (include/kvq.h "beam search")
//
// The 16 waves are split evenly over WT = 1, 2, 4, 8 >= W beam slots (16 / WT waves a beam), so every live beam's row of logits is
// read ONCE, 16 bytes a lane, all beams at the same time.  A thread keeps the WT best raw logits it has seen (sorted, in registers)
// and an online (max, sum exp) of its columns; W rounds of a wave arg-max leave each wave's best W in LDS, a second W rounds over
// the 16 survivors of a beam its best W, and a last W rounds over the at most W * W scored survivors of the sentence the new beams.
// Within a beam the order by logit is the order by score, so no candidate is lost.
// f32 roundings in front of a beam's log-sum-exp, longest chain through one term: its own exponential (2 ulp), the tree of depth 3 over
// the 8 columns of its chunk, then per further chunk of the thread one addition and at most one rescaling of the running sum (a fast
// exponential and a product: 3), then 6 wave levels and the waves of the beam, each an exponential, a product and an addition (4):
// kvq_beam_select refuses a V for which 4 chunks + 5 + 4 (6 + waves) exceeds 256 -- the premise of the tolerance in tests/_beam_ref.py.
// ---------------------------------------------------------------------------------------------------------------
constexpr int BEAM_THREADS = 1024;
constexpr int BEAM_WAVES = BEAM_THREADS / WAVE;
constexpr int BEAM_MAX = 8;
constexpr int BEAM_NONE = 0x7fffffff;

// (m, s) = max and sum exp(x - m) of two disjoint sets of columns; an empty set is (-inf, 0).  Symmetric in its arguments.
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
    const float M = fmaxf(m, om);
    const float a = m == -INFINITY ? 0.f : s * __expf(m - M);
    const float b = om == -INFINITY ? 0.f : os * __expf(om - M);
    m = M;
    s = a + b;
}

template <int DT, int WT>
__global__ __launch_bounds__(BEAM_THREADS) void beam_select_kernel(const GenState* __restrict__ st, const void* __restrict__ logits,
                                                                    int64_t ld, int V, int R, int W, int Lmax, int64_t* __restrict__ ids,
                                                                    int32_t* __restrict__ parent, float* __restrict__ scores,
                                                                    float* __restrict__ step_scores, int32_t* __restrict__ anc,
                                                                    int32_t* __restrict__ finished, int32_t* __restrict__ lengths,
                                                                    float* __restrict__ step_logits) {
    constexpr int WPB = BEAM_WAVES / WT, TPB = WPB * WAVE;     // waves / threads that scan one beam
    __shared__ float old_score[BEAM_MAX];
    __shared__ int old_fin[BEAM_MAX], old_len[BEAM_MAX];
    __shared__ float wave_x[BEAM_MAX][BEAM_WAVES][BEAM_MAX];   // [beam][wave of the beam][rank] (WPB * WT = 16 entries a beam)
    __shared__ int wave_v[BEAM_MAX][BEAM_WAVES][BEAM_MAX];
    __shared__ float wave_m[BEAM_MAX][BEAM_WAVES], wave_s[BEAM_MAX][BEAM_WAVES];
    __shared__ float cand_x[BEAM_MAX][BEAM_MAX];
    __shared__ int cand_v[BEAM_MAX][BEAM_MAX];
    __shared__ int new_parent[BEAM_MAX];                       // the beam (0 .. nW-1) whose history new beam i continues

    const int b = blockIdx.x, r0 = b * W;
    const int nW = min(W, R - r0);                             // (the last sentence of a padded slot space may be short)
    const int t = st->t;
    if (t < 0 || t + 1 >= Lmax || t + 1 >= st->Lmax) return;   // (uniform) no column t + 1: nothing is stored
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pad_id = st->pad_id, eos_id = st->eos_id;
    const size_t half = (size_t)R * Lmax;
    const int32_t* anc_old = anc + (size_t)(t & 1) * half;
    int32_t* anc_new = anc + (size_t)((t + 1) & 1) * half;

    if (t + 1 < st->P) {                                       // (uniform) inside the prompt: tokens, scores and histories are kept
        for (int w = 0; w < nW; ++w) {
            const int r = r0 + w;
            for (int j = tid; j <= t; j += BEAM_THREADS) anc_new[(size_t)r * Lmax + j] = anc_old[(size_t)r * Lmax + j];
            if (tid == 0) {
                anc_new[(size_t)r * Lmax + t + 1] = r;
                parent[(size_t)r * Lmax + t + 1] = r;
                step_scores[(size_t)r * Lmax + t + 1] = scores[r];
            }
            if (step_logits)
                for (int v = tid; v < V; v += BEAM_THREADS) step_logits[((size_t)r * Lmax + t) * V + v] = IO<DT>::load1(logits, (size_t)r * ld + v);
        }
        return;
    }

    // ---- everything of the old state this workgroup will overwrite is read first ----
    if (tid < BEAM_MAX) {
        const bool in = tid < nW;
        old_score[tid] = in ? scores[r0 + tid] : -INFINITY;
        old_fin[tid] = in ? finished[r0 + tid] : 1;
        old_len[tid] = in ? lengths[r0 + tid] : 0;
    }
    __syncthreads();

    // ---- scan: beam `beam` by the waves beam * WPB .. beam * WPB + WPB - 1 ----
    const int beam = wave / WPB, bw = wave - beam * WPB, btid = bw * WAVE + lane;
    const bool live = beam < nW && !old_fin[beam] && old_score[beam] > -INFINITY;      // (uniform per wave)
    if (live) {
        float tv[WT];
        int ti[WT];
#pragma unroll
        for (int k = 0; k < WT; ++k) { tv[k] = -INFINITY; ti[k] = BEAM_NONE; }
        float m = -INFINITY, s = 0.f;
        bool nan = false;
        const size_t row = (size_t)(r0 + beam) * ld;
        float* lrow = step_logits ? step_logits + ((size_t)(r0 + beam) * Lmax + t) * V : nullptr;
        const int nchunk = (V + 7) >> 3;                       // (ld % 8 == 0: the chunk lies inside the row)
#pragma unroll 2
        for (int c = btid; c < nchunk; c += TPB) {
            const f32x8 x8 = IO<DT>::load8(logits, row + 8 * c);
            float x[8] = {x8.lo.x, x8.lo.y, x8.lo.z, x8.lo.w, x8.hi.x, x8.hi.y, x8.hi.z, x8.hi.w};
            float m8 = -INFINITY;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int v = 8 * c + e;
                if (v < V) {
                    if (lrow) lrow[v] = x[e];
                    nan |= x[e] != x[e];
                    m8 = fmaxf(m8, x[e]);
                    if (sel_better(x[e], v, tv[WT - 1], ti[WT - 1])) {      // among the thread's best WT: sorted insertion
                        tv[WT - 1] = x[e]; ti[WT - 1] = v;
#pragma unroll
                        for (int k = WT - 1; k > 0; --k)
                            if (sel_better(tv[k], ti[k], tv[k - 1], ti[k - 1])) {
                                const float fv = tv[k]; tv[k] = tv[k - 1]; tv[k - 1] = fv;
                                const int fi = ti[k]; ti[k] = ti[k - 1]; ti[k - 1] = fi;
                            }
                    }
                } else {
                    x[e] = -INFINITY;                          // (columns >= V never take part)
                }
            }
            if (m8 > m) { s = m == -INFINITY ? 0.f : s * __expf(m - m8); m = m8; }
            if (m > -INFINITY) {
                float e8[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) e8[e] = __expf(x[e] - m);       // (exp(-inf) = 0: a column >= V or a logit of -inf)
                s += ((e8[0] + e8[1]) + (e8[2] + e8[3])) + ((e8[4] + e8[5]) + (e8[6] + e8[7]));
            }
        }
        // the wave's (max, sum): a butterfly, the same bits in every lane
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) {
            const float om = __shfl_xor(m, k, WAVE), os = __shfl_xor(s, k, WAVE);
            lse_merge(m, s, om, os);
        }
        if (__any(nan)) { m = 0.f; s = __builtin_nanf(""); }   // a NaN among the columns: the beam's scores are NaN, it offers nothing
        if (lane == 0) { wave_m[beam][bw] = m; wave_s[beam][bw] = s; }
        // the wave's best W: W rounds of an arg-max over the lanes' heads
        for (int i = 0; i < W; ++i) {
            float bv = tv[0];
            int bi = ti[0];
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) {
                const float ov = __shfl_xor(bv, k, WAVE);
                const int oi = __shfl_xor(bi, k, WAVE);
                if (sel_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (bi != BEAM_NONE && ti[0] == bi) {              // the winner's head leaves its list
#pragma unroll
                for (int k = 0; k + 1 < WT; ++k) { tv[k] = tv[k + 1]; ti[k] = ti[k + 1]; }
                tv[WT - 1] = -INFINITY; ti[WT - 1] = BEAM_NONE;
            }
            if (lane == 0) { wave_x[beam][bw][i] = bv; wave_v[beam][bw][i] = bi; }
        }
    }
    __syncthreads();

    // ---- a beam's best W of its waves' W each: wave w for beam w ----
    if (wave < nW && !old_fin[wave] && old_score[wave] > -INFINITY) {
        const int ww = lane / WT, wi = lane % WT;              // (WPB * WT = 16 lanes hold the survivors)
        float cv = -INFINITY;
        int ci = BEAM_NONE;
        if (ww < WPB && wi < W) { cv = wave_x[wave][ww][wi]; ci = wave_v[wave][ww][wi]; }
        for (int i = 0; i < W; ++i) {
            float bv = cv;
            int bi = ci;
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) {
                const float ov = __shfl_xor(bv, k, WAVE);
                const int oi = __shfl_xor(bi, k, WAVE);
                if (sel_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (bi != BEAM_NONE && ci == bi) { cv = -INFINITY; ci = BEAM_NONE; }
            if (lane == 0) { cand_x[wave][i] = bv; cand_v[wave][i] = bi; }
        }
    }
    __syncthreads();

    // ---- the sentence's best W of the scored survivors: wave 0, lane = (beam, rank) ----
    if (wave == 0) {
        const int w = lane / BEAM_MAX, i = lane % BEAM_MAX;
        float cs = -INFINITY;                                  // the candidate's score; the key of a tie is (beam << 28) | token
        int ck = BEAM_NONE;
        if (w < nW && i < W && old_score[w] > -INFINITY) {
            if (old_fin[w]) {
                if (i == 0) { cs = old_score[w]; ck = w << 28; }            // a finished beam: itself, ranking as (w, 0)
            } else if (cand_v[w][i] != BEAM_NONE) {
                float m = wave_m[w][0], s = wave_s[w][0];
                for (int k = 1; k < WPB; ++k) lse_merge(m, s, wave_m[w][k], wave_s[w][k]);
                const float lse = m + logf(s);
                const float lp = cand_x[w][i] - lse;
                const float sc = old_score[w] + lp;
                if (sc > -INFINITY) { cs = sc; ck = (w << 28) | cand_v[w][i]; }         // (a NaN or -inf score is no candidate)
            }
        }
        float win_s = -INFINITY;
        int win_k = BEAM_NONE;
        for (int n = 0; n < nW; ++n) {
            float bv = cs;
            int bk = ck;
#pragma unroll
            for (int k = 32; k >= 1; k >>= 1) {
                const float ov = __shfl_xor(bv, k, WAVE);
                const int ok = __shfl_xor(bk, k, WAVE);
                if (sel_better(ov, ok, bv, bk)) { bv = ov; bk = ok; }
            }
            if (bk != BEAM_NONE && ck == bk) { cs = -INFINITY; ck = BEAM_NONE; }
            if (lane == n) { win_s = bv; win_k = bk; }
        }
        if (lane < nW) {                                       // new beam `lane` of the sentence
            const int r = r0 + lane;
            const size_t at = (size_t)r * Lmax + t + 1;
            if (win_k == BEAM_NONE) {                          // fewer candidates than beams: a dead beam
                ids[at] = pad_id;
                parent[at] = r;
                scores[r] = -INFINITY;
                step_scores[at] = -INFINITY;
                finished[r] = 1;
                new_parent[lane] = lane;
            } else {
                const int w = win_k >> 28, v = win_k & ((1 << 28) - 1);
                const bool was = old_fin[w] != 0;
                ids[at] = was ? pad_id : v;
                parent[at] = r0 + w;
                scores[r] = win_s;
                step_scores[at] = win_s;
                const bool ends = !was && v == eos_id;
                finished[r] = was || ends ? 1 : 0;
                lengths[r] = ends ? t + 2 : old_len[w];
                new_parent[lane] = w;
            }
        }
    }
    __syncthreads();

    // ---- histories: the parent's row of the old half, extended by the new row itself ----
    for (int i = 0; i < nW; ++i) {
        const int32_t* src = anc_old + (size_t)(r0 + new_parent[i]) * Lmax;
        int32_t* dst = anc_new + (size_t)(r0 + i) * Lmax;
        for (int j = tid; j <= t; j += BEAM_THREADS) dst[j] = src[j];
        if (tid == 0) dst[t + 1] = r0 + i;
    }
}

// hypotheses from slot space: out[r, j] = ids[anc[t & 1][r, j], j] for j < lengths[r] (and j <= t), pad_id behind
__global__ __launch_bounds__(256) void beam_gather_kernel(const GenState* __restrict__ st, const int64_t* __restrict__ ids,
                                                           const int32_t* __restrict__ anc, const int32_t* __restrict__ lengths, int R,
                                                           int Lmax, int64_t* __restrict__ out) {
    const int t = st->t;
    if (t < 0 || t >= Lmax || t >= st->Lmax) return;           // (uniform)
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)R * Lmax) return;
    const int r = (int)(e / Lmax), j = (int)(e - (int64_t)r * Lmax);
    int64_t tok = st->pad_id;
    if (j < lengths[r] && j <= t) {
        const int s = anc[(size_t)(t & 1) * R * Lmax + e];
        tok = ids[(size_t)(s >= 0 && s < R ? s : r) * Lmax + j];
    }
    out[e] = tok;
}

}  // namespace kvq

using namespace kvq;

extern "C" {

int kvq_gen_embed(const void* state, const int64_t* ids, const void* word, const void* pos, const void* type_row, const float* gamma,
                  const float* beta, int B, int H, int64_t V, int pos_rows, float eps, int io_dtype, void* out, void* stream) {
    KVQ_REQUIRE(state && ids && word && pos && type_row && gamma && beta && out, "kvq_gen_embed: null pointer argument");
    KVQ_REQUIRE(B > 0 && H > 0 && V > 0 && pos_rows > 0, "kvq_gen_embed: B, H, V and pos_rows must be positive");
    KVQ_REQUIRE(H % 4 == 0 && H <= 64 * 4 * GEN_LN_MAX_PER_LANE, "kvq_gen_embed: H=%d must be a multiple of 4 and <= 4096", H);
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "kvq_gen_embed: unsupported io dtype %d", io_dtype);
    KVQ_REQUIRE(((uintptr_t)state & 7) == 0 && ((uintptr_t)ids & 7) == 0, "kvq_gen_embed: 8-byte aligned state and ids required");
    KVQ_REQUIRE((((uintptr_t)word | (uintptr_t)pos | (uintptr_t)type_row | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15) == 0
                    && ((size_t)H * (io_dtype == KVQ_BF16 ? 2 : 4)) % 8 == 0,
                "kvq_gen_embed: 16-byte aligned tables, LayerNorm weights and output required");
    hipStream_t s = (hipStream_t)stream;
    const GenState* gs = reinterpret_cast<const GenState*>(state);
    dim3 grid((unsigned)((B + 3) / 4));
    auto with_dt = [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        // (H, io dtype) -> <DT, PER> as ln_dispatch of csrc/kvq_ln.hip maps them: the same chunks per lane, the same sums
        if (H <= 768)
            hipLaunchKernelGGL((gen_embed_kernel<DT, 3>), grid, dim3(256), 0, s, gs, ids, word, pos, type_row, gamma, beta, B, H, V, pos_rows, eps, out);
        else if (H <= 1024)
            hipLaunchKernelGGL((gen_embed_kernel<DT, 4>), grid, dim3(256), 0, s, gs, ids, word, pos, type_row, gamma, beta, B, H, V, pos_rows, eps, out);
        else
            hipLaunchKernelGGL((gen_embed_kernel<DT, GEN_LN_MAX_PER_LANE>), grid, dim3(256), 0, s, gs, ids, word, pos, type_row, gamma, beta, B, H, V,
                               pos_rows, eps, out);
    };
    if (io_dtype == KVQ_F32) with_dt(std::integral_constant<int, KVQ_F32>());
    else with_dt(std::integral_constant<int, KVQ_BF16>());
    return check_launch("gen_embed_kernel");
}

int kvq_gen_attn(const void* state, const void* q, int64_t ldq, const void* k_new, const void* v_new, int64_t ld_new, void* kv,
                 int64_t ld_kv, int64_t kv_sentence_stride, int B, int nh, int append, int n_keys, int Smax, int io_dtype, void* out,
                 int64_t ldo, void* stream) {
    KVQ_REQUIRE(state && q && kv && out, "kvq_gen_attn: null pointer argument");
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "kvq_gen_attn: unsupported io dtype %d", io_dtype);
    KVQ_REQUIRE(B > 0 && nh > 0 && (int64_t)B * nh < (1ll << 31), "kvq_gen_attn: B and nh must be positive (B=%d nh=%d)", B, nh);
    const int64_t W = (int64_t)nh * 64;                                    // columns of q, of the keys and of the values
    const int epl = io_dtype == KVQ_BF16 ? 8 : 4;                          // elements of a 16-byte access
    KVQ_REQUIRE(ldq >= W && ldo >= W && ld_kv >= 2 * W, "kvq_gen_attn: leading dimension below the %lld columns of %d heads", (long long)W, nh);
    KVQ_REQUIRE(ldq % epl == 0 && ldo % epl == 0 && ld_kv % epl == 0 && kv_sentence_stride % epl == 0,
                "kvq_gen_attn: every stride must be a multiple of 16 bytes");
    KVQ_REQUIRE((((uintptr_t)q | (uintptr_t)kv | (uintptr_t)out) & 15) == 0 && ((uintptr_t)state & 7) == 0,
                "kvq_gen_attn: 16-byte aligned q, kv and out (8-byte aligned state) required");
    if (append) {
        KVQ_REQUIRE(k_new && v_new && (((uintptr_t)k_new | (uintptr_t)v_new) & 15) == 0 && ld_new >= W && ld_new % epl == 0,
                    "kvq_gen_attn: append needs 16-byte aligned k_new / v_new rows of at least %lld columns", (long long)W);
        KVQ_REQUIRE(Smax >= 1 && Smax <= GEN_MAX_KEYS, "kvq_gen_attn: Smax=%d outside 1..%d", Smax, GEN_MAX_KEYS);
        KVQ_REQUIRE(kv_sentence_stride >= (int64_t)Smax * ld_kv, "kvq_gen_attn: a sentence of the cache holds fewer than Smax=%d rows", Smax);
    } else {
        KVQ_REQUIRE(n_keys >= 1 && n_keys <= GEN_MAX_KEYS, "kvq_gen_attn: n_keys=%d outside 1..%d", n_keys, GEN_MAX_KEYS);
        KVQ_REQUIRE(kv_sentence_stride >= (int64_t)n_keys * ld_kv, "kvq_gen_attn: a sentence holds fewer than n_keys=%d rows", n_keys);
    }
    hipStream_t s = (hipStream_t)stream;
    const GenState* gs = reinterpret_cast<const GenState*>(state);
    dim3 grid((unsigned)(B * nh));
    if (io_dtype == KVQ_F32)
        hipLaunchKernelGGL(gen_attn_kernel<KVQ_F32>, grid, dim3(64), 0, s, gs, q, ldq, k_new, v_new, ld_new, kv, ld_kv, kv_sentence_stride, nh,
                           append, n_keys, Smax, out, ldo);
    else
        hipLaunchKernelGGL(gen_attn_kernel<KVQ_BF16>, grid, dim3(64), 0, s, gs, q, ldq, k_new, v_new, ld_new, kv, ld_kv, kv_sentence_stride, nh,
                           append, n_keys, Smax, out, ldo);
    return check_launch("gen_attn_kernel");
}

int kvq_gen_select(const void* state, const void* logits, int64_t ld, int V, int B, int io_dtype, int64_t* ids, int32_t* finished, int32_t* lengths, float* step_logits, void* stream) {
    KVQ_REQUIRE(state && logits && ids && finished && lengths, "kvq_gen_select: null pointer argument");
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "kvq_gen_select: unsupported io dtype %d", io_dtype);
    KVQ_REQUIRE(B > 0 && V > 0 && ld >= V, "kvq_gen_select: B, V must be positive and ld >= V (B=%d V=%d ld=%lld)", B, V, (long long)ld);
    KVQ_REQUIRE(ld % 8 == 0 && ((uintptr_t)logits & 15) == 0, "kvq_gen_select: ld %% 8 == 0 and 16-byte aligned logits required");
    KVQ_REQUIRE(((uintptr_t)state & 7) == 0 && ((uintptr_t)ids & 7) == 0 && (((uintptr_t)finished | (uintptr_t)lengths | (uintptr_t)step_logits) & 3) == 0,
                "kvq_gen_select: misaligned state, ids, finished, lengths or step_logits");
    hipStream_t s = (hipStream_t)stream;
    const GenState* gs = reinterpret_cast<const GenState*>(state);
    if (io_dtype == KVQ_F32)
        hipLaunchKernelGGL(gen_select_kernel<KVQ_F32>, dim3((unsigned)B), dim3(SEL_THREADS), 0, s, gs, logits, ld, V, ids, finished, lengths,
                           step_logits);
    else
        hipLaunchKernelGGL(gen_select_kernel<KVQ_BF16>, dim3((unsigned)B), dim3(SEL_THREADS), 0, s, gs, logits, ld, V, ids, finished, lengths,
                           step_logits);
    return check_launch("gen_select_kernel");
}

int kvq_gen_select_filtered(const void* state, const void* filter, const void* logits, int64_t ld, int V, int B, int io_dtype, int64_t* ids,
                            int32_t* finished, int32_t* lengths, float* step_logits, int32_t* step_kept, int32_t* step_cut,
                            float* step_logprob, void* stream) {
    KVQ_REQUIRE(state && filter && logits && ids && finished && lengths, "kvq_gen_select_filtered: null pointer argument");
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "kvq_gen_select_filtered: unsupported io dtype %d", io_dtype);
    KVQ_REQUIRE(B > 0 && V > 0 && ld >= V, "kvq_gen_select_filtered: B, V must be positive and ld >= V (B=%d V=%d ld=%lld)", B, V, (long long)ld);
    KVQ_REQUIRE(V <= FLT_MAX_V, "kvq_gen_select_filtered: V=%d above the %d columns a workgroup holds in registers", V, FLT_MAX_V);
    KVQ_REQUIRE(ld % 8 == 0 && ((uintptr_t)logits & 15) == 0, "kvq_gen_select_filtered: ld %% 8 == 0 and 16-byte aligned logits required");
    KVQ_REQUIRE(((uintptr_t)state & 7) == 0 && ((uintptr_t)filter & 3) == 0 && ((uintptr_t)ids & 7) == 0
                    && (((uintptr_t)finished | (uintptr_t)lengths | (uintptr_t)step_logits | (uintptr_t)step_kept | (uintptr_t)step_cut
                         | (uintptr_t)step_logprob) & 3) == 0,
                "kvq_gen_select_filtered: misaligned state, filter, ids or int32 / f32 buffers");
    hipStream_t s = (hipStream_t)stream;
    const GenState* gs = reinterpret_cast<const GenState*>(state);
    const GenFilter* fs = reinterpret_cast<const GenFilter*>(filter);
    if (io_dtype == KVQ_F32)
        hipLaunchKernelGGL(gen_select_filtered_kernel<KVQ_F32>, dim3((unsigned)B), dim3(FLT_THREADS), 0, s, gs, fs, logits, ld, V, ids, finished,
                           lengths, step_logits, step_kept, step_cut, step_logprob);
    else
        hipLaunchKernelGGL(gen_select_filtered_kernel<KVQ_BF16>, dim3((unsigned)B), dim3(FLT_THREADS), 0, s, gs, fs, logits, ld, V, ids, finished,
                           lengths, step_logits, step_kept, step_cut, step_logprob);
    return check_launch("gen_select_filtered_kernel");
}

int kvq_beam_attn(const void* state, const void* q, int64_t ldq, const void* k_new, const void* v_new, int64_t ld_new, void* kv,
                  int64_t ld_kv, int64_t kv_sentence_stride, int R, int nh, int append, int n_keys, int Smax, const int32_t* anc,
                  int anc_ld, int rows_per_sentence, int io_dtype, void* out, int64_t ldo, void* stream) {
    KVQ_REQUIRE(state && q && kv && out, "kvq_beam_attn: null pointer argument");
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "kvq_beam_attn: unsupported io dtype %d", io_dtype);
    KVQ_REQUIRE(R > 0 && nh > 0 && (int64_t)R * nh < (1ll << 31), "kvq_beam_attn: R and nh must be positive (R=%d nh=%d)", R, nh);
    const int64_t W = (int64_t)nh * 64;
    const int epl = io_dtype == KVQ_BF16 ? 8 : 4;
    KVQ_REQUIRE(ldq >= W && ldo >= W && ld_kv >= 2 * W, "kvq_beam_attn: leading dimension below the %lld columns of %d heads", (long long)W, nh);
    KVQ_REQUIRE(ldq % epl == 0 && ldo % epl == 0 && ld_kv % epl == 0 && kv_sentence_stride % epl == 0,
                "kvq_beam_attn: every stride must be a multiple of 16 bytes");
    KVQ_REQUIRE((((uintptr_t)q | (uintptr_t)kv | (uintptr_t)out) & 15) == 0 && ((uintptr_t)state & 7) == 0,
                "kvq_beam_attn: 16-byte aligned q, kv and out (8-byte aligned state) required");
    if (append) {
        KVQ_REQUIRE(k_new && v_new && (((uintptr_t)k_new | (uintptr_t)v_new) & 15) == 0 && ld_new >= W && ld_new % epl == 0,
                    "kvq_beam_attn: append needs 16-byte aligned k_new / v_new rows of at least %lld columns", (long long)W);
        KVQ_REQUIRE(Smax >= 1 && Smax <= GEN_MAX_KEYS, "kvq_beam_attn: Smax=%d outside 1..%d", Smax, GEN_MAX_KEYS);
        KVQ_REQUIRE(kv_sentence_stride >= (int64_t)Smax * ld_kv, "kvq_beam_attn: a row of the cache holds fewer than Smax=%d positions", Smax);
        KVQ_REQUIRE(anc && ((uintptr_t)anc & 3) == 0 && anc_ld >= Smax, "kvq_beam_attn: append needs the ancestry table [2, R, anc_ld >= Smax=%d]", Smax);
    } else {
        KVQ_REQUIRE(n_keys >= 1 && n_keys <= GEN_MAX_KEYS, "kvq_beam_attn: n_keys=%d outside 1..%d", n_keys, GEN_MAX_KEYS);
        KVQ_REQUIRE(kv_sentence_stride >= (int64_t)n_keys * ld_kv, "kvq_beam_attn: a sentence holds fewer than n_keys=%d rows", n_keys);
        KVQ_REQUIRE(rows_per_sentence >= 1, "kvq_beam_attn: rows_per_sentence=%d must be positive", rows_per_sentence);
    }
    hipStream_t s = (hipStream_t)stream;
    const GenState* gs = reinterpret_cast<const GenState*>(state);
    dim3 grid((unsigned)(R * nh));
    const int64_t half = (int64_t)R * anc_ld;
    if (io_dtype == KVQ_F32)
        hipLaunchKernelGGL(beam_attn_kernel<KVQ_F32>, grid, dim3(64), 0, s, gs, q, ldq, k_new, v_new, ld_new, kv, ld_kv, kv_sentence_stride, nh,
                           append, n_keys, Smax, out, ldo, anc, half, anc_ld, rows_per_sentence, R);
    else
        hipLaunchKernelGGL(beam_attn_kernel<KVQ_BF16>, grid, dim3(64), 0, s, gs, q, ldq, k_new, v_new, ld_new, kv, ld_kv, kv_sentence_stride, nh,
                           append, n_keys, Smax, out, ldo, anc, half, anc_ld, rows_per_sentence, R);
    return check_launch("beam_attn_kernel");
}

int kvq_beam_select(const void* state, const void* logits, int64_t ld, int V, int R, int W, int Lmax, int io_dtype, int64_t* ids,
                    int32_t* parent, float* scores, float* step_scores, int32_t* anc, int32_t* finished, int32_t* lengths,
                    float* step_logits, void* stream) {
    KVQ_REQUIRE(state && logits && ids && parent && scores && step_scores && anc && finished && lengths, "kvq_beam_select: null pointer argument");
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "kvq_beam_select: unsupported io dtype %d", io_dtype);
    KVQ_REQUIRE(R > 0 && V > 0 && ld >= V && Lmax > 0, "kvq_beam_select: R, V, Lmax must be positive and ld >= V (R=%d V=%d ld=%lld)", R, V, (long long)ld);
    KVQ_REQUIRE(W >= 1 && W <= BEAM_MAX && W <= V, "kvq_beam_select: W=%d outside 1..%d or above V=%d", W, BEAM_MAX, V);
    KVQ_REQUIRE(ld % 8 == 0 && ((uintptr_t)logits & 15) == 0, "kvq_beam_select: ld %% 8 == 0 and 16-byte aligned logits required");
    KVQ_REQUIRE(((uintptr_t)state & 7) == 0 && ((uintptr_t)ids & 7) == 0
                    && (((uintptr_t)parent | (uintptr_t)scores | (uintptr_t)step_scores | (uintptr_t)anc | (uintptr_t)finished | (uintptr_t)lengths
                         | (uintptr_t)step_logits) & 3) == 0,
                "kvq_beam_select: misaligned state, ids or int32 / f32 buffers");
    const int WT = W <= 1 ? 1 : W <= 2 ? 2 : W <= 4 ? 4 : 8, waves = BEAM_WAVES / WT;
    const int chunks = ((V + 7) / 8 + waves * WAVE - 1) / (waves * WAVE);          // of one thread
    KVQ_REQUIRE(V < (1 << 28) && 4 * chunks + 5 + 4 * (6 + waves) <= 256,
                "kvq_beam_select: V=%d with W=%d puts more than 256 roundings in front of a log-sum-exp (the bound of its tolerance)", V, W);
    hipStream_t s = (hipStream_t)stream;
    const GenState* gs = reinterpret_cast<const GenState*>(state);
    dim3 grid((unsigned)((R + W - 1) / W));
    auto go = [&](auto dt, auto wt) {
        constexpr int DT = decltype(dt)::value, WTc = decltype(wt)::value;
        hipLaunchKernelGGL((beam_select_kernel<DT, WTc>), grid, dim3(BEAM_THREADS), 0, s, gs, logits, ld, V, R, W, Lmax, ids, parent, scores, step_scores,
                           anc, finished, lengths, step_logits);
    };
    auto with_dt = [&](auto dt) {
        if (WT == 1) go(dt, std::integral_constant<int, 1>());
        else if (WT == 2) go(dt, std::integral_constant<int, 2>());
        else if (WT == 4) go(dt, std::integral_constant<int, 4>());
        else go(dt, std::integral_constant<int, 8>());
    };
    if (io_dtype == KVQ_F32) with_dt(std::integral_constant<int, KVQ_F32>());
    else with_dt(std::integral_constant<int, KVQ_BF16>());
    return check_launch("beam_select_kernel");
}

int kvq_beam_gather(const void* state, const int64_t* ids, const int32_t* anc, const int32_t* lengths, int R, int Lmax, int64_t* out,
                    void* stream) {
    KVQ_REQUIRE(state && ids && anc && lengths && out, "kvq_beam_gather: null pointer argument");
    KVQ_REQUIRE(R > 0 && Lmax > 0, "kvq_beam_gather: R and Lmax must be positive (R=%d Lmax=%d)", R, Lmax);
    KVQ_REQUIRE(((uintptr_t)state & 7) == 0 && (((uintptr_t)ids | (uintptr_t)out) & 7) == 0 && (((uintptr_t)anc | (uintptr_t)lengths) & 3) == 0,
                "kvq_beam_gather: misaligned buffers");
    const int64_t n = (int64_t)R * Lmax;
    hipLaunchKernelGGL(beam_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const GenState*>(state), ids, anc, lengths, R, Lmax, out);
    return check_launch("beam_gather_kernel");
}

int kvq_gen_advance(void* state, void* stream) {
    KVQ_REQUIRE(state && ((uintptr_t)state & 7) == 0, "kvq_gen_advance: null / misaligned generation state");
    hipLaunchKernelGGL(gen_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (GenState*)state);
    return check_launch("gen_advance_kernel");
}

int kvq_gen_gumbel_debug(const uint32_t* bits, int64_t n, float* out, void* stream) {
    KVQ_REQUIRE(bits && out && n > 0 && n < (1ll << 31), "kvq_gen_gumbel_debug: bad argument");
    KVQ_REQUIRE((((uintptr_t)bits | (uintptr_t)out) & 3) == 0, "kvq_gen_gumbel_debug: misaligned buffers");
    hipLaunchKernelGGL(gen_gumbel_debug_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bits, n, out);
    return check_launch("gen_gumbel_debug_kernel");
}

}  // extern "C"
