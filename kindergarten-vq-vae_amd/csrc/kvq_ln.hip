// kvq_ln.hip -- the LayerNorm family of the training step, fused for gfx950 (bf16 or f32 storage, f32 arithmetic).
//
// The reference runs these as separate ATen ops inside HuggingFace's BertLayer / BertEmbeddings (modeling_bert.py): bias add,
// dropout, residual add and LayerNorm.  Here each is one pass over the activations:
//   kvq_dropout_residual_ln_fwd{,_fp8}   BertSelfOutput / BertOutput (:282-293, :340-352): LN(dropout(y) + residual)
//   kvq_embed_ln_fwd                     BertEmbeddings (:53-110): dropout(LN(word[ids] + pos + type))
//   kvq_dropout_residual_ln_bwd{,_partial}, kvq_ln_dropout_bwd_partial   their backward, dgamma / dbeta / dense-bias partials per workgroup
// Four kernels: drln_fwd_kernel, embed_ln_fwd_kernel, and the backward schedule written once (ln_bwd_body) behind the two kernel
// names the host chooses between, drln_bwd_kernel (8 bytes of bf16 per lane and access, any H) and drln_bwd16_kernel (16 bytes).
// Dropout masks are never stored: both directions regenerate them from Philox4x32-10 keyed by (seed, site) and indexed by the
// element position, ONE call per 4 consecutive elements (kvq_common.h; the GEMM epilogue of csrc/kvq_gemm2.hip draws the same masks).
#include <math.h>

#include "kvq_common.h"
#include <type_traits>

namespace kvq {

constexpr int LN_MAX_PER_LANE = 16;   // H <= 64 * 4 * 16 = 4096

// ---- four lanes (one quad = 4 consecutive elements) at a time.  -ffp-contract=off: the order of the sums is the source's ------
// (the helpers update the lanes of their by-value argument instead of building a vector: that form keeps the kernels on the schedule
// they were measured with, profiles/ln_one_body.md)
template <int DT>
__device__ __forceinline__ f32x4 round4(f32x4 v) {               // the values a consumer of the stored quad reads back
    v.x = IO<DT>::round(v.x); v.y = IO<DT>::round(v.y); v.z = IO<DT>::round(v.z); v.w = IO<DT>::round(v.w);
    return v;
}
template <int DT>
__device__ __forceinline__ f32x4 add_rounded4(f32x4 acc, f32x4 v) {   // acc + round4(v)
    acc.x += IO<DT>::round(v.x); acc.y += IO<DT>::round(v.y); acc.z += IO<DT>::round(v.z); acc.w += IO<DT>::round(v.w);
    return acc;
}
__device__ __forceinline__ float quadsum(f32x4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
// a quad times its keep scales: from its 4 x 32 random bits (forward), from 4 keep bits (backward: drawn while the loads fly, used twice)
__device__ __forceinline__ f32x4 keep_scale4(f32x4 v, U4 b, unsigned thresh, float inv_keep) {
    v.x *= keep_scale(b.x, thresh, inv_keep); v.y *= keep_scale(b.y, thresh, inv_keep);
    v.z *= keep_scale(b.z, thresh, inv_keep); v.w *= keep_scale(b.w, thresh, inv_keep);
    return v;
}
__device__ __forceinline__ unsigned keep_bits4(U4 b, unsigned thresh) {
    return (b.x >= thresh ? 1u : 0u) | (b.y >= thresh ? 2u : 0u) | (b.z >= thresh ? 4u : 0u) | (b.w >= thresh ? 8u : 0u);
}
__device__ __forceinline__ f32x4 keep4(f32x4 v, unsigned bits, float inv_keep) {
    v.x *= (bits & 1u) ? inv_keep : 0.f; v.y *= (bits & 2u) ? inv_keep : 0.f;
    v.z *= (bits & 4u) ? inv_keep : 0.f; v.w *= (bits & 8u) ? inv_keep : 0.f;
    return v;
}

// ---------------------------------------------------------------------------------------------------------------
// forward: one wave per row, rows of H <= 4096 (H % 4 == 0), lane `lane` holds the chunks lane + 64 t of 4 elements
// ---------------------------------------------------------------------------------------------------------------
// row statistics from the lanes' sums: mean, a quad's squared deviations (the caller masks the chunks past the row), rstd
__device__ __forceinline__ float ln_mean(float sum, int H) { return wave_sum_f32(sum) / (float)H; }
__device__ __forceinline__ float ln_sqdev(f32x4 v, float mean) {
    const f32x4 d = v - mean;
    return dot4(d, d);
}
__device__ __forceinline__ float ln_rstd(float sq, int H, float eps) {
    const float var = wave_sum_f32(sq) / (float)H;
    return rsqrtf(var + eps);
}
__device__ __forceinline__ void ln_store_stats(int lane, int64_t row, float mean, float rstd, float* mean_out, float* rstd_out) {
    if (lane == 0) {
        if (mean_out) mean_out[row] = mean;
        if (rstd_out) rstd_out[row] = rstd;
    }
}

// LN(dropout(y) + residual).  RES = false: no residual operand at all -- the LayerNorm-only pass behind kvq_gemm_bf16_dropres,
// whose GEMM epilogue already added the residual: one load stream instead of two.
template <int DT, int PER, bool RES = true>
__global__ __launch_bounds__(256) void drln_fwd_kernel(const void* __restrict__ y, const void* __restrict__ resid,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        int64_t N, int H, float eps, float p_drop, unsigned thresh,
                                                        unsigned long long seed, const unsigned long long* __restrict__ seed_off,
                                                        unsigned site, void* __restrict__ out,
                                                        void* __restrict__ pre, float* __restrict__ mean_out,
                                                        float* __restrict__ rstd_out, unsigned char* __restrict__ out8 = nullptr,
                                                        float* __restrict__ st8 = nullptr) {
    // out8 / st8 (bf16 io only): also the fp8 (e4m3) copy of `out` for the fp8 GEMM that reads it next -- the bytes
    // kvq_fp8_quantize_delayed(out) would write (this site's scale of the previous step, this call's amax noted in its state)
    // EVERY load of the row is requested before anything is done with one of them, and no load sits behind a branch: chunk
    // indices past the row are clamped (and masked out of the sums), a missing residual reads y again and is weighted 0.
    // As first written ("if (c < nchunk) { load y; ...; if (resid) load resid; ... }" per chunk) hipcc put s_waitcnt vmcnt(0)
    // behind each load: six dependent trips to memory per row, then three more for gamma / beta -- 13.3 us for the 50 MB of a
    // [8192, 768] call, one round of waves doing nothing but waiting (ISA audit, profiles/NOTES_r01-r03_design_and_experiments.md section 2.5).
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int nchunk = H >> 2;
    const float inv_keep = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
    const void* rp = resid ? resid : y;
    const float rw = resid ? 1.0f : 0.0f;
    constexpr bool EARLY_GB = PER <= 4;        // (wide rows: gamma / beta stay L2-resident small loads of the last pass)
    f32x4 v[PER], r[RES ? PER : 1], g[EARLY_GB ? PER : 1], b[EARLY_GB ? PER : 1];
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int c = lane + WAVE * t < nchunk ? lane + WAVE * t : nchunk - 1;
        const size_t off = (size_t)row * H + 4 * c;
        v[t] = IO<DT>::load4(y, off);
        if constexpr (RES) r[t] = IO<DT>::load4(rp, off);
    }
    if constexpr (EARLY_GB) {
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            const int c = lane + WAVE * t < nchunk ? lane + WAVE * t : nchunk - 1;
            g[t] = *reinterpret_cast<const f32x4*>(gamma + 4 * c);
            b[t] = *reinterpret_cast<const f32x4*>(beta + 4 * c);
        }
    }
    if (seed_off) seed += *seed_off;          // device-resident step counter (a captured graph replays with fresh masks): the
                                              // dependent scalar load waits while the row is on its way
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int c = lane + WAVE * t;
        f32x4 a = v[t];
        if (p_drop > 0.f) {                   // (uniform; arithmetic only: the Philox rounds run while the loads are in flight)
            const U4 kb = drop_bits(seed, site, (unsigned long long)row * nchunk + c);
            a = keep_scale4(a, kb, thresh, inv_keep);
        }
        if constexpr (RES) a += r[t] * rw;
        // LayerNorm sees the STORED pre-activation (bf16-rounded when io is bf16): backward re-reads exactly that
        v[t] = round4<DT>(a);
        if (c < nchunk) {
            if (pre) IO<DT>::store4(pre, (size_t)row * H + 4 * c, v[t]);
            sum += quadsum(v[t]);
        }
    }
    const float mean = ln_mean(sum, H);
    float sq = 0.f;
#pragma unroll
    for (int t = 0; t < PER; ++t)
        if (lane + WAVE * t < nchunk) sq += ln_sqdev(v[t], mean);
    const float rstd = ln_rstd(sq, H, eps);
    const float s8 = (DT == KVQ_BF16 && out8) ? st8[0] : 1.0f;
    float am8 = 0.f;
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int c = lane + WAVE * t;
        if (c < nchunk) {
            f32x4 gg, bb;
            if constexpr (EARLY_GB) { gg = g[t]; bb = b[t]; }
            else { gg = *reinterpret_cast<const f32x4*>(gamma + 4 * c); bb = *reinterpret_cast<const f32x4*>(beta + 4 * c); }
            const f32x4 o = (v[t] - mean) * rstd * gg + bb;
            IO<DT>::store4(out, (size_t)row * H + 4 * c, o);
            if (DT == KVQ_BF16 && out8) {                     // (uniform)
                const f32x4 ob = round4<DT>(o);
                am8 = fmaxf(am8, amax4(ob));
                *reinterpret_cast<unsigned*>(out8 + (size_t)row * H + 4 * c) = quant4(ob, s8);
            }
        }
    }
    if (DT == KVQ_BF16 && out8) fp8_amax_note(am8, st8, (unsigned)row);
    ln_store_stats(lane, row, mean, rstd, mean_out, rstd_out);
}

// BertEmbeddings (modeling_bert.py:53-110) in one pass: out = dropout(LayerNorm(word[ids[n]] + (pos[n % S] + type[0]))).
// Replaces F.embedding + the position/type add + its repeat over the batch + the LayerNorm kernel + the dropout kernel (five
// launches, three [N, H] round trips).  Rounding as those kernels rounded: pos + type to the io dtype, the sum to the io dtype
// (= `pre`, what backward re-reads), the LayerNorm output to the io dtype BEFORE the keep scale.  One wave per row; the gathers
// sit under `c < nchunk` (a load schedule of its own, on purpose).
template <int DT, int PER>
__global__ __launch_bounds__(256) void embed_ln_fwd_kernel(const int64_t* __restrict__ ids, const void* __restrict__ word,
                                                            const void* __restrict__ pos, const void* __restrict__ type_row,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            int64_t N, int S, int H, int64_t V, float eps, float p_drop, unsigned thresh,
                                                            unsigned long long seed, const unsigned long long* __restrict__ seed_off,
                                                            unsigned site, void* __restrict__ out, void* __restrict__ pre,
                                                            float* __restrict__ mean_out, float* __restrict__ rstd_out) {
    if (seed_off) seed += *seed_off;
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const int nchunk = H >> 2;
    int64_t id = ids[row];
    id = id < 0 ? 0 : (id >= V ? V - 1 : id);                 // (torch raises on an id outside the table; the kernel must not fault)
    const int ps = (int)(row % S);
    const float inv_keep = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
    f32x4 v[PER];
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int c = lane + WAVE * t;
        f32x4 a = {0.f, 0.f, 0.f, 0.f};
        if (c < nchunk) {
            f32x4 pt = IO<DT>::load4(pos, (size_t)ps * H + 4 * c) + IO<DT>::load4(type_row, 4 * c);
            pt = round4<DT>(pt);
            a = IO<DT>::load4(word, (size_t)id * H + 4 * c) + pt;
            // (round4 here moves the bf16 kernels off the measured schedule -- profiles/ln_one_body.md -- so this quad is rounded in place)
            a.x = IO<DT>::round(a.x); a.y = IO<DT>::round(a.y); a.z = IO<DT>::round(a.z); a.w = IO<DT>::round(a.w);
            if (pre) IO<DT>::store4(pre, (size_t)row * H + 4 * c, a);
            sum += quadsum(a);
        }
        v[t] = a;
    }
    const float mean = ln_mean(sum, H);
    float sq = 0.f;
#pragma unroll
    for (int t = 0; t < PER; ++t)
        if (lane + WAVE * t < nchunk) sq += ln_sqdev(v[t], mean);
    const float rstd = ln_rstd(sq, H, eps);
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int c = lane + WAVE * t;
        if (c < nchunk) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + 4 * c);
            const f32x4 b = *reinterpret_cast<const f32x4*>(beta + 4 * c);
            f32x4 o = (v[t] - mean) * rstd * g + b;
            if (p_drop > 0.f)
                o = keep_scale4(round4<DT>(o), drop_bits(seed, site, (unsigned long long)row * nchunk + c), thresh, inv_keep);
            IO<DT>::store4(out, (size_t)row * H + 4 * c, o);
        }
    }
    ln_store_stats(lane, row, mean, rstd, mean_out, rstd_out);
}

// ---------------------------------------------------------------------------------------------------------------
// backward: g_pre = rstd * (g*gamma - mean(g*gamma) - xhat * mean(g*gamma*xhat));  g_resid = g_pre;
//           g_y = g_pre * dropout_mask/(1-p);  dgamma/dbeta partials per workgroup (summed by kvq_reduce_batch)
// ---------------------------------------------------------------------------------------------------------------
constexpr int LNB_ROWS = 16;   // rows per workgroup, all in flight at once where the registers allow: 512 workgroups and 512 partial rows at N = 8192

__device__ __forceinline__ float half_wave_sum_f32(float v) {
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}
template <int LANES>
__device__ __forceinline__ float row_sum_f32(float v) {          // over the LANES lanes that share a row
    static_assert(LANES == WAVE || LANES == WAVE / 2, "a wave or half a wave per row");
    return LANES == WAVE ? wave_sum_f32(v) : half_wave_sum_f32(v);
}

// VEC consecutive elements = VEC / 4 quads per lane and access (VEC = 8: bf16, 16-byte aligned, off % 8 == 0)
template <int DT, int VEC>
__device__ __forceinline__ void load_quads(const void* base, size_t off, f32x4 (&q)[VEC / 4]) {
    if constexpr (VEC == 4) {
        q[0] = IO<DT>::load4(base, off);
    } else {
        const f32x8 v = IO<DT>::load8(base, off);
        q[0] = v.lo; q[1] = v.hi;
    }
}
template <int DT, int VEC>
__device__ __forceinline__ void store_quads(void* base, size_t off, const f32x4 (&q)[VEC / 4]) {
    if constexpr (VEC == 4) {
        IO<DT>::store4(base, off, q[0]);
    } else {
        const f32x8 v = {q[0], q[1]};
        IO<DT>::store8(base, off, v);
    }
}

// The schedule of both backward kernels.  A group of 64 * 4 / VEC lanes shares a row (VEC = 4: a wave, 8 bytes of bf16 per lane and
// access; VEC = 8: HALF a wave, 16 bytes -- in the step 16.7 -> 14.3 us per [8192, 768] call; the forward kernel rebuilt the same
// way measured 13.3 against 13.4 us and was dropped again: it is not the access width that holds it), lane l of it holds the
// chunks l + LANES t of VEC elements, H <= VEC * LANES * PER.  Which form runs is the host's choice (ln_bwd_partial_impl).
// drop_on_out: the block is dropout(LayerNorm(.)) (BertEmbeddings) instead of LayerNorm(dropout(y) + resid): the mask of
// (seed, site) then applies to the incoming gradient g_out (rounded to the io dtype, as the separate kernel stored it).
template <int DT, int PER, int VEC>
__device__ __forceinline__ void ln_bwd_body(const void* __restrict__ g_out, const void* __restrict__ pre,
                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                            const float* __restrict__ gamma, int64_t N, int H, float p_drop, unsigned thresh,
                                            unsigned long long seed, const unsigned long long* __restrict__ seed_off, unsigned site,
                                            void* __restrict__ g_y, void* __restrict__ g_resid, float* __restrict__ part_dgamma,
                                            int want_dbias, int drop_on_out) {
    static_assert(VEC == 4 || VEC == 8, "one or two quads per access");
    extern __shared__ __attribute__((aligned(16))) float lds[];   // [4 waves][3][H]
    if (seed_off) seed += *seed_off;
    constexpr int Q = VEC / 4;                                    // quads per access
    constexpr int LANES = WAVE / Q;                               // lanes per row
    constexpr int RW = LNB_ROWS / (256 / LANES);                  // rows per lane group: 4 or 2
    constexpr int RF = (Q == 2 || PER <= 4) ? RW : 1;             // ... of which RF are in flight at once (register budget)
    typedef typename std::conditional<(4 * Q * PER > 32), unsigned long long, unsigned>::type KeepBits;   // 4 bits per quad
    const int ll = threadIdx.x & (LANES - 1), grp = threadIdx.x / LANES, w = threadIdx.x >> 6;
    const int nquad = H >> 2, nchunk = H >> (VEC == 8 ? 3 : 2);     // chunks of 4 and of VEC elements in a row
    const float inv_keep = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
    f32x4 dg[PER][Q], db[PER][Q], dy[PER][Q], gm[PER][Q];         // dy: column sums of g_y = bias gradient of the dense layer in front
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int c = ll + LANES * t < nchunk ? ll + LANES * t : nchunk - 1;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            dg[t][q] = 0.f; db[t][q] = 0.f; dy[t][q] = 0.f;
            gm[t][q] = *reinterpret_cast<const f32x4*>(gamma + VEC * c + 4 * q);
        }
    }
#pragma unroll
    for (int rb = 0; rb < RW; rb += RF) {
        const int64_t row0 = (int64_t)blockIdx.x * LNB_ROWS + grp * RW + rb;
        if (LANES == WAVE && row0 >= N) break;                    // a whole wave with nothing left to do
        // 1. every load of these rows goes out first (rows past N are clamped and weighted 0: no branch around a load)
        f32x4 go[RF][PER][Q], x[RF][PER][Q];
        float mu[RF], rs[RF], live[RF];
#pragma unroll
        for (int r = 0; r < RF; ++r) {
            const int64_t row = row0 + r < N ? row0 + r : N - 1;
            live[r] = row0 + r < N ? 1.0f : 0.0f;
            mu[r] = mean[row]; rs[r] = rstd[row];
#pragma unroll
            for (int t = 0; t < PER; ++t) {
                const int c = ll + LANES * t < nchunk ? ll + LANES * t : nchunk - 1;
                const size_t off = (size_t)row * H + VEC * c;
                load_quads<DT, VEC>(g_out, off, go[r][t]);
                load_quads<DT, VEC>(pre, off, x[r][t]);
            }
        }
        // 2. the dropout keep bits do not depend on the loads: Philox runs while they are in flight (one call per quad)
        KeepBits keepbits[RF];
#pragma unroll
        for (int r = 0; r < RF; ++r) {
            keepbits[r] = ~(KeepBits)0;
            if ((g_y || drop_on_out) && p_drop > 0.f) {
                KeepBits kb = 0;
#pragma unroll
                for (int t = 0; t < PER; ++t) {
                    const int c = ll + LANES * t;
#pragma unroll
                    for (int q = 0; q < Q; ++q)
                        kb |= (KeepBits)keep_bits4(drop_bits(seed, site, (unsigned long long)(row0 + r) * nquad + Q * c + q), thresh) << (4 * (Q * t + q));
                }
                keepbits[r] = kb;
            }
        }
        // 3. row statistics of all rows in flight, then their outputs
        float s1[RF], s2[RF];
#pragma unroll
        for (int r = 0; r < RF; ++r) {
            float a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int t = 0; t < PER; ++t) {
                const float m = (ll + LANES * t < nchunk) ? live[r] : 0.0f;
                if constexpr (Q == 1) {
                    // one quad per access: this statement order is the one the 256-VGPR instantiations (PER = 16) were measured with; the
                    // per-quad arrays of the other arm cost drln_bwd_kernel<f32, 16> 16 more bytes of scratch (profiles/ln_one_body.md)
                    f32x4 g = go[r][t][0] * m;
                    if (drop_on_out) g = round4<DT>(keep4(g, (unsigned)(keepbits[r] >> (4 * t)), inv_keep));
                    const f32x4 xh = (x[r][t][0] - mu[r]) * rs[r];
                    const f32x4 tt = g * gm[t][0];
                    dg[t][0] += g * xh;
                    db[t][0] += g;
                    a1 += quadsum(tt);
                    a2 += dot4(tt, xh);
                    go[r][t][0] = tt; x[r][t][0] = xh;
                } else {
                    f32x4 g[Q];
#pragma unroll
                    for (int q = 0; q < Q; ++q) g[q] = go[r][t][q] * m;
                    if (drop_on_out) {
                        const unsigned kb = (unsigned)(keepbits[r] >> (4 * Q * t));
#pragma unroll
                        for (int q = 0; q < Q; ++q) g[q] = round4<DT>(keep4(g[q], kb >> (4 * q), inv_keep));
                    }
                    float q1[Q], q2[Q];
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        const f32x4 xh = (x[r][t][q] - mu[r]) * rs[r];
                        const f32x4 tt = g[q] * gm[t][q];
                        dg[t][q] += g[q] * xh;
                        db[t][q] += g[q];
                        q1[q] = quadsum(tt);
                        q2[q] = dot4(tt, xh);
                        go[r][t][q] = tt; x[r][t][q] = xh;
                    }
                    a1 += q1[0] + q1[1];                           // the two quads of an access first, then the running sum
                    a2 += q2[0] + q2[1];
                }
            }
            s1[r] = a1; s2[r] = a2;
        }
#pragma unroll
        for (int r = 0; r < RF; ++r) {
            s1[r] = row_sum_f32<LANES>(s1[r]) / (float)H;
            s2[r] = row_sum_f32<LANES>(s2[r]) / (float)H;
        }
#pragma unroll
        for (int r = 0; r < RF; ++r) {
            if (row0 + r >= N) break;                    // uniform over the lane group; only stores below
#pragma unroll
            for (int t = 0; t < PER; ++t) {
                const int c = ll + LANES * t;
                if (c < nchunk) {
                    const size_t off = (size_t)(row0 + r) * H + VEC * c;
                    f32x4 gp[Q];
#pragma unroll
                    for (int q = 0; q < Q; ++q) gp[q] = (go[r][t][q] - s1[r] - x[r][t][q] * s2[r]) * rs[r];
                    if (g_resid) store_quads<DT, VEC>(g_resid, off, gp);
                    if (g_y) {
                        if (!drop_on_out) {
                            const unsigned kb = (unsigned)(keepbits[r] >> (4 * Q * t));
#pragma unroll
                            for (int q = 0; q < Q; ++q) gp[q] = keep4(gp[q], kb >> (4 * q), inv_keep);
                        }
                        store_quads<DT, VEC>(g_y, off, gp);
                        // what the consumer of g_y reads back is the STORED (possibly bf16-rounded) value
#pragma unroll
                        for (int q = 0; q < Q; ++q) dy[t][q] = add_rounded4<DT>(dy[t][q], gp[q]);
                    }
                }
            }
        }
    }
    // lane groups of one wave hold the same columns: add them, then the 4 waves through LDS
    float* l_dy = lds + (size_t)w * 3 * H;
    float* l_dg = l_dy + H;
    float* l_db = l_dg + H;
#pragma unroll
    for (int t = 0; t < PER; ++t) {
        const int c = ll + LANES * t;
        if constexpr (LANES < WAVE) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    dy[t][q][j] += __shfl_xor(dy[t][q][j], 32, WAVE); dg[t][q][j] += __shfl_xor(dg[t][q][j], 32, WAVE);
                    db[t][q][j] += __shfl_xor(db[t][q][j], 32, WAVE);
                }
            }
        }
        if ((threadIdx.x & (WAVE - LANES)) == 0 && c < nchunk) {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                *reinterpret_cast<f32x4*>(l_dy + VEC * c + 4 * q) = dy[t][q];
                *reinterpret_cast<f32x4*>(l_dg + VEC * c + 4 * q) = dg[t][q];
                *reinterpret_cast<f32x4*>(l_db + VEC * c + 4 * q) = db[t][q];
            }
        }
    }
    __syncthreads();
    // partial row layout: [dbias_prev(H) | dgamma(H) | dbeta(H)], the waves summed 0..3
    for (int j = threadIdx.x; j < 3 * H; j += 256) {
        if (j < H && !want_dbias) continue;
        float a = 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) a += lds[(size_t)ww * 3 * H + j];
        part_dgamma[(size_t)blockIdx.x * 3 * H + j] = a;
    }
}

template <int DT, int PER>
__global__ __launch_bounds__(256) void drln_bwd_kernel(const void* __restrict__ g_out, const void* __restrict__ pre,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        const float* __restrict__ gamma, int64_t N, int H, float p_drop,
                                                        unsigned thresh, unsigned long long seed,
                                                        const unsigned long long* __restrict__ seed_off, unsigned site,
                                                        void* __restrict__ g_y, void* __restrict__ g_resid,
                                                        float* __restrict__ part_dgamma, int want_dbias, int drop_on_out) {
    ln_bwd_body<DT, PER, 4>(g_out, pre, mean, rstd, gamma, N, H, p_drop, thresh, seed, seed_off, site, g_y, g_resid, part_dgamma,
                            want_dbias, drop_on_out);
}

// bf16 io, H % 8 == 0, H <= 8 * 32 * PER, every pointer 16-byte aligned
template <int PER>
__global__ __launch_bounds__(256) void drln_bwd16_kernel(const void* __restrict__ g_out, const void* __restrict__ pre,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, int64_t N, int H, float p_drop,
                                                          unsigned thresh, unsigned long long seed,
                                                          const unsigned long long* __restrict__ seed_off, unsigned site,
                                                          void* __restrict__ g_y, void* __restrict__ g_resid,
                                                          float* __restrict__ part_dgamma, int want_dbias, int drop_on_out) {
    ln_bwd_body<KVQ_BF16, PER, 8>(g_out, pre, mean, rstd, gamma, N, H, p_drop, thresh, seed, seed_off, site, g_y, g_resid, part_dgamma,
                                  want_dbias, drop_on_out);
}

}  // namespace kvq

using namespace kvq;

// (H, io dtype) -> launch(dt, per) with the instantiation's <DT, PER> as the values of two integral constants
template <class F>
static void ln_dispatch(int H, int io_dtype, F&& launch) {
    auto with_dt = [&](auto dt) {
        if (H <= 768) launch(dt, std::integral_constant<int, 3>());
        else if (H <= 1024) launch(dt, std::integral_constant<int, 4>());
        else launch(dt, std::integral_constant<int, LN_MAX_PER_LANE>());
    };
    if (io_dtype == KVQ_F32) with_dt(std::integral_constant<int, KVQ_F32>());
    else with_dt(std::integral_constant<int, KVQ_BF16>());
}

extern "C" {

static int drln_fwd_impl(const void* y, const void* resid, const float* gamma, const float* beta, int64_t N, int H,
                         float eps, float p_drop, uint64_t seed, uint32_t site, int io_dtype, void* out, void* pre,
                         float* mean, float* rstd, unsigned char* out8, float* st8, void* stream) {
    KVQ_REQUIRE(y && gamma && beta && out && N > 0 && H > 0, "kvq_dropout_residual_ln_fwd: bad argument");
    KVQ_REQUIRE(H % 4 == 0 && H <= 64 * 4 * LN_MAX_PER_LANE, "kvq_dropout_residual_ln_fwd: H=%d must be a multiple of 4 and <= 4096", H);
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "unsupported io dtype %d", io_dtype);
    KVQ_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "p_drop out of range");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)((N + 3) / 4));
    const unsigned th = drop_threshold(p_drop);
    if (!resid && H <= 768 && io_dtype == KVQ_BF16) {          // LayerNorm alone (the dense layer's epilogue added the residual)
        hipLaunchKernelGGL((drln_fwd_kernel<KVQ_BF16, 3, false>), grid, dim3(256), 0, st, y, resid, gamma, beta, N, H, eps, p_drop, th,
                           (unsigned long long)seed, seed_offset_ptr(), site, out, pre, mean, rstd, out8, st8);
    } else {
        ln_dispatch(H, io_dtype, [&](auto dt, auto per) {
            hipLaunchKernelGGL((drln_fwd_kernel<decltype(dt)::value, decltype(per)::value>), grid, dim3(256), 0, st, y, resid, gamma, beta,
                               N, H, eps, p_drop, th, (unsigned long long)seed, seed_offset_ptr(), site, out, pre, mean, rstd, out8, st8);
        });
    }
    return check_launch("drln_fwd_kernel");
}

int kvq_dropout_residual_ln_fwd(const void* y, const void* resid, const float* gamma, const float* beta, int64_t N, int H,
                                float eps, float p_drop, uint64_t seed, uint32_t site, int io_dtype, void* out, void* pre,
                                float* mean, float* rstd, void* stream) {
    return drln_fwd_impl(y, resid, gamma, beta, N, H, eps, p_drop, seed, site, io_dtype, out, pre, mean, rstd, nullptr, nullptr, stream);
}

int kvq_dropout_residual_ln_fwd_fp8(const void* y, const void* resid, const float* gamma, const float* beta, int64_t N, int H,
                                    float eps, float p_drop, uint64_t seed, uint32_t site, void* out, void* pre, float* mean, float* rstd,
                                    void* out_fp8, float* fp8_state, void* stream) {
    KVQ_REQUIRE(out_fp8 && fp8_state && ((uintptr_t)out_fp8 & 3) == 0, "kvq_dropout_residual_ln_fwd_fp8: null / misaligned fp8 output or state");
    return drln_fwd_impl(y, resid, gamma, beta, N, H, eps, p_drop, seed, site, KVQ_BF16, out, pre, mean, rstd, (unsigned char*)out_fp8, fp8_state, stream);
}

int kvq_embed_ln_fwd(const int64_t* ids, const void* word, const void* pos, const void* type_row, const float* gamma,
                     const float* beta, int64_t N, int S, int H, int64_t V, float eps, float p_drop, uint64_t seed, uint32_t site,
                     int io_dtype, void* out, void* pre, float* mean, float* rstd, void* stream) {
    KVQ_REQUIRE(ids && word && pos && type_row && gamma && beta && out && N > 0 && S > 0 && H > 0 && V > 0, "kvq_embed_ln_fwd: bad argument");
    KVQ_REQUIRE(H % 4 == 0 && H <= 64 * 4 * LN_MAX_PER_LANE, "kvq_embed_ln_fwd: H=%d must be a multiple of 4 and <= 4096", H);
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "unsupported io dtype %d", io_dtype);
    KVQ_REQUIRE(p_drop >= 0.f && p_drop < 1.f, "p_drop out of range");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)((N + 3) / 4));
    const unsigned th = drop_threshold(p_drop);
    ln_dispatch(H, io_dtype, [&](auto dt, auto per) {
        hipLaunchKernelGGL((embed_ln_fwd_kernel<decltype(dt)::value, decltype(per)::value>), grid, dim3(256), 0, st, ids, word, pos, type_row,
                           gamma, beta, N, S, H, V, eps, p_drop, th, (unsigned long long)seed, seed_offset_ptr(), site, out, pre, mean, rstd);
    });
    return check_launch("embed_ln_fwd_kernel");
}

int64_t kvq_ln_bwd_partial_rows(int64_t N) { return (N + LNB_ROWS - 1) / LNB_ROWS; }

size_t kvq_ln_bwd_workspace_bytes(int64_t N, int H) { return (size_t)kvq_ln_bwd_partial_rows(N) * H * 3 * sizeof(float); }

static int ln_bwd_partial_impl(const void* g_out, const void* pre, const float* mean, const float* rstd,
                               const float* gamma, int64_t N, int H, float p_drop, uint64_t seed, uint32_t site,
                               int io_dtype, void* g_y, void* g_resid, int want_dbias, void* part, size_t part_bytes,
                               void* stream, int drop_on_out) {
    KVQ_REQUIRE(g_out && pre && mean && rstd && gamma && N > 0 && H > 0, "kvq_dropout_residual_ln_bwd: bad argument");
    KVQ_REQUIRE(H % 4 == 0 && H <= 3072, "kvq_dropout_residual_ln_bwd: H=%d unsupported (multiple of 4, <= 3072: 48*H bytes of LDS)", H);
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "unsupported io dtype %d", io_dtype);
    const size_t need = kvq_ln_bwd_workspace_bytes(N, H);
    if (!part || part_bytes < need) return fail(KVQ_E_WORKSPACE, "kvq_dropout_residual_ln_bwd: workspace %zu < %zu", part_bytes, need);
    KVQ_REQUIRE(!want_dbias || g_y, "kvq_dropout_residual_ln_bwd: the dense-bias partials need g_y");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)kvq_ln_bwd_partial_rows(N));
    const size_t lds = (size_t)4 * 3 * H * sizeof(float);
    const unsigned th = drop_threshold(p_drop);
    // one argument list for both kernels
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, g_out, pre, mean, rstd, gamma, N, H, p_drop, th, (unsigned long long)seed,
                           seed_offset_ptr(), site, g_y, g_resid, (float*)part, want_dbias ? 1 : 0, drop_on_out);
    };
    if (io_dtype == KVQ_BF16 && H % 8 == 0 && H <= 1024 && H >= 64 && LNB_ROWS % 8 == 0 &&
        ((((uintptr_t)g_out | (uintptr_t)pre | (uintptr_t)g_y | (uintptr_t)g_resid | (uintptr_t)gamma) & 15) == 0)) {
        if (H <= 256) launch(drln_bwd16_kernel<1>);
        else if (H <= 512) launch(drln_bwd16_kernel<2>);
        else if (H <= 768) launch(drln_bwd16_kernel<3>);
        else launch(drln_bwd16_kernel<4>);
        return check_launch("drln_bwd16_kernel");
    }
    ln_dispatch(H, io_dtype, [&](auto dt, auto per) { launch(drln_bwd_kernel<decltype(dt)::value, decltype(per)::value>); });
    return check_launch("drln_bwd_kernel");
}

int kvq_dropout_residual_ln_bwd_partial(const void* g_out, const void* pre, const float* mean, const float* rstd,
                                        const float* gamma, int64_t N, int H, float p_drop, uint64_t seed, uint32_t site,
                                        int io_dtype, void* g_y, void* g_resid, int want_dbias, void* part, size_t part_bytes,
                                        void* stream) {
    return ln_bwd_partial_impl(g_out, pre, mean, rstd, gamma, N, H, p_drop, seed, site, io_dtype, g_y, g_resid, want_dbias, part,
                               part_bytes, stream, 0);
}

int kvq_ln_dropout_bwd_partial(const void* g_out, const void* pre, const float* mean, const float* rstd, const float* gamma,
                               int64_t N, int H, float p_drop, uint64_t seed, uint32_t site, int io_dtype, void* g_y,
                               void* part, size_t part_bytes, void* stream) {
    return ln_bwd_partial_impl(g_out, pre, mean, rstd, gamma, N, H, p_drop, seed, site, io_dtype, g_y, nullptr, 0, part, part_bytes,
                               stream, 1);
}

int kvq_dropout_residual_ln_bwd(const void* g_out, const void* pre, const float* mean, const float* rstd, const float* gamma,
                                int64_t N, int H, float p_drop, uint64_t seed, uint32_t site, int io_dtype, void* g_y,
                                void* g_resid, void* g_gamma, void* g_beta, void* g_bias_prev, int param_grad_dtype, int accumulate,
                                void* ws, size_t ws_bytes, void* stream) {
    int rc = kvq_dropout_residual_ln_bwd_partial(g_out, pre, mean, rstd, gamma, N, H, p_drop, seed, site, io_dtype, g_y, g_resid,
                                                 g_bias_prev ? 1 : 0, ws, ws_bytes, stream);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t blocks = kvq_ln_bwd_partial_rows(N);
    float* pdg = (float*)ws;
    const size_t esz = param_grad_dtype == KVQ_F32 ? 4 : 2;
    const int64_t H3 = 3 * (int64_t)H;
    const bool gb_adj = g_gamma && g_beta && (char*)g_beta == (char*)g_gamma + (size_t)H * esz;
    const bool all_adj = gb_adj && g_bias_prev && (char*)g_gamma == (char*)g_bias_prev + (size_t)H * esz;
    if (all_adj) {
        // [dense bias | LN weight | LN bias] are adjacent in the engine's flat layout: ONE pass writes all three
        rc = colsum_f32_partials(pdg, blocks, H3, H3, g_bias_prev, param_grad_dtype, 1.0f, accumulate, st);
        if (rc) return rc;
    } else {
        if (g_bias_prev) { rc = colsum_f32_partials(pdg, blocks, H, H3, g_bias_prev, param_grad_dtype, 1.0f, accumulate, st); if (rc) return rc; }
        if (gb_adj) {
            rc = colsum_f32_partials(pdg + H, blocks, 2 * (int64_t)H, H3, g_gamma, param_grad_dtype, 1.0f, accumulate, st);
            if (rc) return rc;
        } else {
            if (g_gamma) { rc = colsum_f32_partials(pdg + H, blocks, H, H3, g_gamma, param_grad_dtype, 1.0f, accumulate, st); if (rc) return rc; }
            if (g_beta) { rc = colsum_f32_partials(pdg + 2 * H, blocks, H, H3, g_beta, param_grad_dtype, 1.0f, accumulate, st); if (rc) return rc; }
        }
    }
    return KVQ_OK;
}

}  // extern "C"
