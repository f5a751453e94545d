// kvq_seqcmp.hip -- free-running reconstruction metrics on gfx950: per sentence the token edit distance
// (Levenshtein, unit costs), the positional matches and the two lengths of a generated sentence against its reference, and the sums
// of those per table row (all sentences, one row per generative-factor value).
//
// What teacher-forced accuracy (kvq_seq_acc) cannot see: a sentence that comes back with one word dropped or inserted has every
// later position shifted, so its positional count collapses while its edit distance is 1.
//
// Neither kernel is on the training step.  Integers only: the same inputs give the same bits in any order of execution.
#include "kvq_common.h"

namespace kvq {

constexpr int SEQ_MAX = 128;          // tokens per side at most: two reference columns per lane of one wavefront
constexpr int SEQ_WAVES = 4;          // pairs per workgroup, one wavefront each
constexpr int SEQ_THREADS = SEQ_WAVES * WAVE;
constexpr int ACC_THREADS = 256;

// ---------------------------------------------------------------------------------------------------------------
// kvq_seq_compare.  One wavefront per pair.  D[i][j] = distance of the first i hypothesis tokens to the first j reference tokens,
//     D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + (h[i-1] != r[j-1])).
// Lane l owns the reference columns j = l + 1 (group 0) and j = l + 65 (group 1) with their tokens in registers; the hypothesis
// sits in LDS.  The table is walked by anti-diagonals d = i + j = 2 .. n + m (a wave-uniform trip count of n + m - 1): on
// diagonal d column j holds row i = d - j, and its three inputs are
//     up   = D[i-1][j]    its own value on diagonal d - 1                       (v[g]; starts as the boundary D[0][j] = j)
//     left = D[i][j-1]    its left neighbour's value on diagonal d - 1           (one rotation of the packed pair of values)
//     diag = D[i-1][j-1]  its left neighbour's value on diagonal d - 2 = the `left` it fetched one diagonal earlier.
// The left neighbour of lane l > 0 is lane l - 1 in the same group.  Seams: lane 0 of group 0 borders column 0 (left = D[i][0] =
// d - 1, diag = d - 2); lane 0 of group 1 (column 65) borders column 64 = lane 63 of group 0.  Both values of a lane travel in one
// dword (each <= 256), rotated by one lane, so lane 0 receives lane 63's pair and takes its group-0 half.
// A column is updated only while 1 <= i <= n, so after the last diagonal column m still holds D[n][m].
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SEQ_THREADS) void seq_compare_kernel(const int64_t* __restrict__ hyp, int64_t ld_hyp, int hyp_skip,
                                                                  const int32_t* __restrict__ hyp_len, const int64_t* __restrict__ ref,
                                                                  int64_t ld_ref, const int32_t* __restrict__ ref_len, int64_t B, int Lmax,
                                                                  int32_t* __restrict__ out, unsigned long long* __restrict__ n_bad) {
    __shared__ int64_t h_tok[SEQ_WAVES][SEQ_MAX];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int64_t b = (int64_t)blockIdx.x * SEQ_WAVES + wave;
    const bool have = b < B;
    // the lengths as the device holds them; a row whose lengths do not fit is answered (-1, 0, 0, 0) and counted, never read
    const int64_t n64 = have ? (int64_t)hyp_len[b] - hyp_skip : 0, m64 = have ? (int64_t)ref_len[b] : 0;
    const bool fits = n64 >= 0 && n64 <= Lmax && m64 >= 0 && m64 <= Lmax && hyp_skip + n64 <= ld_hyp && m64 <= ld_ref;
    const int n = __builtin_amdgcn_readfirstlane(fits ? (int)n64 : 0), m = __builtin_amdgcn_readfirstlane(fits ? (int)m64 : 0);
    const int64_t* h = hyp + (have ? b : 0) * ld_hyp + hyp_skip;
    const int64_t* r = ref + (have ? b : 0) * ld_ref;
    int64_t rt[2], ht[2];
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int c = lane + WAVE * g;
        rt[g] = c < m ? r[c] : 0;
        ht[g] = c < n ? h[c] : 0;
        h_tok[wave][c] = ht[g];
    }
    __syncthreads();
    if (!have) return;
    if (!fits) {
        if (lane == 0) {
            *reinterpret_cast<int4*>(out + 4 * b) = make_int4(-1, 0, 0, 0);
            atomicAdd(n_bad, 1ull);
        }
        return;
    }
    // positional matches over the common prefix
    const int common = n < m ? n : m;
    int hits = 0;
#pragma unroll
    for (int g = 0; g < 2; ++g) hits += (lane + WAVE * g < common && rt[g] == ht[g]) ? 1 : 0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) hits += __shfl_xor(hits, o, WAVE);

    int dist;
    if (n == 0 || m == 0) {
        dist = n > m ? n : m;
    } else {
        int v[2] = {lane + 1, lane + 1 + WAVE};              // D[0][j]
        int diag[2] = {lane, lane + WAVE};                   // D[0][j-1]
        const int src = (lane + WAVE - 1) & (WAVE - 1);
        for (int d = 2; d <= n + m; ++d) {
            const int rot = __shfl(v[0] | (v[1] << 16), src, WAVE);
            int left[2];
            left[0] = lane == 0 ? d - 1 : (rot & 0xffff);
            left[1] = lane == 0 ? (rot & 0xffff) : (rot >> 16);
            if (lane == 0) diag[0] = d - 2;
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const int j = lane + 1 + WAVE * g, i = d - j;
                if (j <= m && i >= 1 && i <= n) {
                    const int sub = diag[g] + (h_tok[wave][i - 1] != rt[g] ? 1 : 0);
                    const int step = (v[g] < left[g] ? v[g] : left[g]) + 1;
                    v[g] = sub < step ? sub : step;
                }
                diag[g] = left[g];
            }
        }
        const int own = m - 1;                               // column m: lane own & 63, group own >> 6
        dist = __shfl(own >= WAVE ? v[1] : v[0], own & (WAVE - 1), WAVE);
    }
    if (lane == 0) *reinterpret_cast<int4*>(out + 4 * b) = make_int4(dist, hits, n, m);
}

// ---------------------------------------------------------------------------------------------------------------
// kvq_seq_compare_accumulate.  One item = one (sentence, slot column): table[slot] += (1, dist == 0, dist, hits, n, m) with
// 64-bit integer atomics (exact and order-free).  Items are laid out column-major over the sentences, so a wave reads consecutive
// rows of `per`.
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ACC_THREADS) void seq_accumulate_kernel(const int32_t* __restrict__ per, int64_t B, const int32_t* __restrict__ slot,
                                                                     int C, int64_t R, unsigned long long* __restrict__ table) {
    const int64_t item = (int64_t)blockIdx.x * ACC_THREADS + threadIdx.x;
    if (item >= B * C) return;
    const int64_t b = item % B;
    const int c = (int)(item / B);
    const int4 p = *reinterpret_cast<const int4*>(per + 4 * b);          // (dist, hits, n, m)
    const int64_t s = slot[b * C + c];
    if (p.x < 0 || s < 0 || s >= R) return;
    unsigned long long* t = table + 6 * s;
    atomicAdd(t + 0, 1ull);
    if (p.x == 0) atomicAdd(t + 1, 1ull);
    if (p.x) atomicAdd(t + 2, (unsigned long long)p.x);
    if (p.y) atomicAdd(t + 3, (unsigned long long)p.y);
    if (p.z) atomicAdd(t + 4, (unsigned long long)p.z);
    if (p.w) atomicAdd(t + 5, (unsigned long long)p.w);
}

}  // namespace kvq

using namespace kvq;

extern "C" {

int kvq_seq_compare(const int64_t* hyp, int64_t ld_hyp, int hyp_skip, const int32_t* hyp_len, const int64_t* ref, int64_t ld_ref,
                    const int32_t* ref_len, int64_t B, int Lmax, int32_t* out, int64_t* n_bad, void* stream) {
    KVQ_REQUIRE(B >= 0, "kvq_seq_compare: B >= 0 required (B=%lld)", (long long)B);
    KVQ_REQUIRE(Lmax >= 0 && Lmax <= SEQ_MAX, "kvq_seq_compare: Lmax must be in 0 .. %d, got %d", SEQ_MAX, Lmax);
    KVQ_REQUIRE(hyp_skip >= 0, "kvq_seq_compare: hyp_skip must be >= 0, got %d", hyp_skip);
    KVQ_REQUIRE(ld_hyp >= 0 && ld_ref >= 0, "kvq_seq_compare: row strides %lld, %lld must be >= 0", (long long)ld_hyp, (long long)ld_ref);
    KVQ_REQUIRE(hyp && hyp_len && ref && ref_len && out && n_bad, "kvq_seq_compare: null pointer argument");
    KVQ_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)n_bad & 7) == 0, "kvq_seq_compare: out must be 16-byte, n_bad 8-byte aligned");
    if (B == 0) return KVQ_OK;
    const int64_t blocks = (B + SEQ_WAVES - 1) / SEQ_WAVES;
    KVQ_REQUIRE(blocks < (int64_t)1 << 31, "kvq_seq_compare: %lld workgroups do not fit one launch", (long long)blocks);
    hipLaunchKernelGGL(seq_compare_kernel, dim3((unsigned)blocks), dim3(SEQ_THREADS), 0, (hipStream_t)stream, hyp, ld_hyp, hyp_skip, hyp_len,
                       ref, ld_ref, ref_len, B, Lmax, out, (unsigned long long*)n_bad);
    return check_launch("seq_compare_kernel");
}

int kvq_seq_compare_accumulate(const int32_t* per, int64_t B, const int32_t* slot, int C, int64_t R, int64_t* table, void* stream) {
    KVQ_REQUIRE(B >= 0, "kvq_seq_compare_accumulate: B >= 0 required (B=%lld)", (long long)B);
    KVQ_REQUIRE(C >= 1 && C <= 16, "kvq_seq_compare_accumulate: C must be in 1 .. 16, got %d", C);
    KVQ_REQUIRE(R >= 1 && R <= 4096, "kvq_seq_compare_accumulate: R must be in 1 .. 4096, got %lld", (long long)R);
    KVQ_REQUIRE(per && slot && table, "kvq_seq_compare_accumulate: null pointer argument");
    KVQ_REQUIRE(((uintptr_t)per & 15) == 0 && ((uintptr_t)table & 7) == 0,
                "kvq_seq_compare_accumulate: per must be 16-byte, table 8-byte aligned");
    if (B == 0) return KVQ_OK;
    const int64_t blocks = (B * C + ACC_THREADS - 1) / ACC_THREADS;
    KVQ_REQUIRE(blocks < (int64_t)1 << 31, "kvq_seq_compare_accumulate: %lld workgroups do not fit one launch", (long long)blocks);
    hipLaunchKernelGGL(seq_accumulate_kernel, dim3((unsigned)blocks), dim3(ACC_THREADS), 0, (hipStream_t)stream, per, B, slot, C, R,
                       (unsigned long long*)table);
    return check_launch("seq_accumulate_kernel");
}

}  // extern "C"
