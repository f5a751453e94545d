// kvq_adam.hip -- the optimiser update of the training step and the device-resident step state it reads (gfx950).
//
//   kvq_adam_step                      torch.optim.Adam (main.py:91: coupled L2 weight decay, optional amsgrad) on flat buffers: p32
//                                      (master, f32), g (bf16 or f32), m, v (f32) [, vmax], shadow (bf16 copy of p32 for the next forward)
//   kvq_adam_step_dev[_fp8]            lr and the bias corrections read from the step state [the fp8 weight mirror written as well]
//   kvq_adam_step_guarded[_fp8]        behind the step's gradient guard (csrc/kvq_gradnorm.hip)
//   kvq_adam_step_grouped[_guarded]    a learning-rate scale and a weight decay per parameter group, optionally decoupled (AdamW)
//   kvq_step_state_advance[_sched]     step += 1, the learning rate and the bias corrections of that step
//
// The update schedule is written ONCE (adam_body); what the entry points differ in are its compile-time arms.  The two kernels
// only call it: adam_kernel<DT_G> for the entries without groups, adam_group_kernel<DT_G, TABLE, DEC> for the grouped ones.
#include <math.h>

#include "kvq_common.h"

namespace kvq {

// DEC (torch.optim.AdamW's decoupled decay): p0 = fl(p * keep) with keep = fl(1 - fl(lr_j * wd_j)) formed where the group is known,
// then the coupled statements with wd = 0: g * c + p0 * 0 has the value of g * c, so the moments see the gradient alone.
template <bool DEC>
__device__ __forceinline__ void adam_update4(f32x4& pv, f32x4 gv, f32x4& mv, f32x4& vv, float* vmax4, float lr, float b1, float b2,
                                             float eps, float wd, float keep, float bc1, float bc2_sqrt) {
    if (DEC) {
        pv = pv * keep;
        wd = 0.0f;
    }
    gv += pv * wd;
    mv = mv * b1 + gv * (1.0f - b1);
    vv = vv * b2 + (gv * gv) * (1.0f - b2);
    f32x4 den_src = vv;
    if (vmax4) {
        f32x4 vm = *reinterpret_cast<f32x4*>(vmax4);
        vm.x = fmaxf(vm.x, vv.x); vm.y = fmaxf(vm.y, vv.y); vm.z = fmaxf(vm.z, vv.z); vm.w = fmaxf(vm.w, vv.w);
        *reinterpret_cast<f32x4*>(vmax4) = vm;
        den_src = vm;
    }
    f32x4 den;
    den.x = sqrtf(den_src.x) / bc2_sqrt + eps; den.y = sqrtf(den_src.y) / bc2_sqrt + eps;
    den.z = sqrtf(den_src.z) / bc2_sqrt + eps; den.w = sqrtf(den_src.w) / bc2_sqrt + eps;
    const float step = lr / bc1;
    pv.x -= step * (mv.x / den.x); pv.y -= step * (mv.y / den.y);
    pv.z -= step * (mv.z / den.z); pv.w -= step * (mv.w / den.w);
}

// Optional (fp8 forward GEMMs): the fp8 (e4m3) mirror of the GEMM weights written by the update itself, from the bf16 value
// it has just rounded for the shadow -- instead of a conversion pass over the whole shadow buffer after every step.  The mirror is
// indexed like the flat parameter buffer (one byte per element); `gseg[global element >> 11]` names the quantisation segment (= GEMM
// weight, one scale each) that covers a 2048-element span: >= 0 the segment, -1 none, -2 more than one thing (the thread then walks
// the segment table).  Segments start and end at multiples of 16 elements, so a thread's 8 elements never straddle one.
struct AdamFp8 {
    unsigned char* w8;            // null: no mirror
    const int* gseg;
    const float* scale;           // [nseg] current scales (kvq_fp8_quantize_segments*)
    const int64_t* seg_off;       // [nseg] first element of each segment
    const int64_t* seg_n;         // [nseg]
    int nseg;
    int64_t e_base;               // global element index of p[0]
};

// Where the rate and the decay of an element come from.  With a table, bgroup[(e_base + e) >> 4] names the group of each 16-element
// block of the flat buffer (FlatParams starts and pads every entry at multiples of 16, so a thread's 8 elements share one byte); the
// <= 16 entries of both tables sit in LDS, the rate already scaled: lr_j = fl(lr * s_j).  A group id is masked to 0 .. 15: a table
// byte can never index outside the LDS arrays.
enum AdamGroups {
    ADAM_NO_GROUPS,               // lr and wd of the launch
    ADAM_ONE_GROUP,               // entry 0 of both tables for the whole launch, read once per thread (uniform)
    ADAM_GROUP_TABLE
};

// The update of one launch.  8 parameters per thread and pass: every array moves in 16-byte accesses (the bf16 gradient and shadow
// included), two independent 4-element updates in flight.  n8 = n / 8 chunks; a tail of 4 (n % 8 == 4) is handled by the last thread.
//   DT_G     the gradient's dtype
//   GROUPS   AdamGroups.  Without groups `hyper` (lr, bc1, bc2_sqrt of the step state) may be null: kvq_adam_step passes them by value.
//   DEC      decoupled decay (adam_update4), with groups only
//   MIRROR   the launch may carry an fp8 mirror (f8.w8, a uniform run-time test); false: no code for it
template <int DT_G, int GROUPS, bool DEC, bool MIRROR>
__device__ __forceinline__ void adam_body(float* __restrict__ p, const void* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                          float* __restrict__ vmax, unsigned short* __restrict__ shadow, int64_t n4, int n_tail,
                                          float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt, float grad_scale,
                                          const float* __restrict__ hyper, const GradGuard* __restrict__ guard, AdamFp8 f8,
                                          const unsigned char* __restrict__ bgroup, int64_t e_base, const float* __restrict__ g_scale,
                                          const float* __restrict__ g_wd, int n_groups) {
    static_assert(GROUPS != ADAM_NO_GROUPS || !DEC, "the decoupled decay is an arm of the grouped forms");
    __shared__ float s_lr[16], s_wd[16];
    if (guard) {                                                           // the step's gradient guard (uniform)
        if (guard->skip) return;                                           // non-finite gradient: nothing is stored, nothing decays
        grad_scale *= guard->coef;                                         // the clipping coefficient of kvq_grad_guard_finalize
    }
    float lr1 = lr, wd1 = wd, keep1 = 1.0f;                                // of the chunk's group; keep1: the decoupled decay's factor
    if constexpr (GROUPS == ADAM_NO_GROUPS) {
        if (hyper) { lr1 = hyper[0]; bc1 = hyper[1]; bc2_sqrt = hyper[2]; }   // device-resident step state (kvq_step_state_advance)
    } else {
        // The table loads are unconditional, from an address that is valid either way (a NULL table reads word 0 of the step state's
        // floats and drops the value): they are issued together with the step state's instead of one round trip behind it and a
        // branch -- every wave runs this prologue (profiles/adam_groups.md).
        const float* sp = g_scale ? g_scale : hyper;
        const float* wp = g_wd ? g_wd : hyper;
        lr = hyper[0]; bc1 = hyper[1]; bc2_sqrt = hyper[2];
        const float s0 = sp[0], w0 = wp[0];
        lr1 = lr * (g_scale ? s0 : 1.0f);
        wd1 = g_wd ? w0 : wd;
        if constexpr (GROUPS == ADAM_ONE_GROUP) {
            // both are uniform, but the product and the select are vector instructions, and their results (and the copies the packed
            // arithmetic wants) would sit in vector registers.  Read back into scalar registers they are what lr and wd are without
            // groups (78 instead of 84 VGPRs).
            lr1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(lr1)));
            wd1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wd1)));
            keep1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(1.0f - lr1 * wd1)));
        } else {
            if (threadIdx.x < 16) {
                const int j = threadIdx.x, jj = j < n_groups ? j : 0;
                const float sj = sp[g_scale ? jj : 0], wj = wp[g_wd ? jj : 0];       // (a NULL table stands in with ONE valid word)
                s_lr[j] = j < n_groups ? lr * (g_scale ? sj : 1.0f) : 0.0f;
                s_wd[j] = j < n_groups ? (g_wd ? wj : wd) : 0.0f;
            }
            __syncthreads();
        }
    }
    auto pick_group = [&](int64_t e) {                                     // the group of the 16-element block that holds element e
        if constexpr (GROUPS == ADAM_GROUP_TABLE) {
            const int j = bgroup[(e_base + e) >> 4] & 15;
            lr1 = s_lr[j]; wd1 = s_wd[j]; keep1 = 1.0f - lr1 * wd1;
        }
    };
    const int64_t n8 = n4 >> 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        const int64_t e = 8 * i;
        pick_group(e);
        f32x4 p0 = *reinterpret_cast<f32x4*>(p + e), p1 = *reinterpret_cast<f32x4*>(p + e + 4);
        f32x4 m0 = *reinterpret_cast<f32x4*>(m + e), m1 = *reinterpret_cast<f32x4*>(m + e + 4);
        f32x4 v0 = *reinterpret_cast<f32x4*>(v + e), v1 = *reinterpret_cast<f32x4*>(v + e + 4);
        const f32x8 gv = IO<DT_G>::load8(g, e);
        adam_update4<DEC>(p0, gv.lo * grad_scale, m0, v0, vmax ? vmax + e : nullptr, lr1, b1, b2, eps, wd1, keep1, bc1, bc2_sqrt);
        adam_update4<DEC>(p1, gv.hi * grad_scale, m1, v1, vmax ? vmax + e + 4 : nullptr, lr1, b1, b2, eps, wd1, keep1, bc1, bc2_sqrt);
        *reinterpret_cast<f32x4*>(p + e) = p0; *reinterpret_cast<f32x4*>(p + e + 4) = p1;
        *reinterpret_cast<f32x4*>(m + e) = m0; *reinterpret_cast<f32x4*>(m + e + 4) = m1;
        *reinterpret_cast<f32x4*>(v + e) = v0; *reinterpret_cast<f32x4*>(v + e + 4) = v1;
        if (shadow) { f32x8 o = {p0, p1}; IO<KVQ_BF16>::store8(shadow, e, o); }
        if (MIRROR && f8.w8) {                                              // (uniform)
            const int64_t ge = f8.e_base + e;
            int sg = f8.gseg[ge >> 11];
            if (sg == -2) {
                sg = -1;
                for (int q = 0; q < f8.nseg; ++q)
                    if (ge >= f8.seg_off[q] && ge < f8.seg_off[q] + f8.seg_n[q]) sg = q;
            }
            if (sg >= 0) {
                const uint4 r = {(unsigned)f32_to_bf16(p0.x) | ((unsigned)f32_to_bf16(p0.y) << 16), (unsigned)f32_to_bf16(p0.z) | ((unsigned)f32_to_bf16(p0.w) << 16),
                                 (unsigned)f32_to_bf16(p1.x) | ((unsigned)f32_to_bf16(p1.y) << 16), (unsigned)f32_to_bf16(p1.z) | ((unsigned)f32_to_bf16(p1.w) << 16)};
                *reinterpret_cast<uint2*>(f8.w8 + ge) = quant8(r, f8.scale[sg]);
            }
        }
    }
    if ((n4 & 1) && blockIdx.x == 0 && threadIdx.x == 0) {                  // the odd 4-element chunk
        const int64_t e = 4 * (n4 - 1);
        pick_group(e);
        f32x4 pv = *reinterpret_cast<f32x4*>(p + e), mv = *reinterpret_cast<f32x4*>(m + e), vv = *reinterpret_cast<f32x4*>(v + e);
        adam_update4<DEC>(pv, IO<DT_G>::load4(g, e) * grad_scale, mv, vv, vmax ? vmax + e : nullptr, lr1, b1, b2, eps, wd1, keep1, bc1,
                          bc2_sqrt);
        *reinterpret_cast<f32x4*>(p + e) = pv; *reinterpret_cast<f32x4*>(m + e) = mv; *reinterpret_cast<f32x4*>(v + e) = vv;
        if (shadow) IO<KVQ_BF16>::store4(shadow, e, pv);
    }
    if (n_tail && blockIdx.x == 0 && threadIdx.x == 1) {                    // 1 .. 3 last elements (9-code Gumbel bias, ...): one block
        const int64_t e0 = 4 * n4;                                          // (they follow a multiple of 4)
        pick_group(e0);
        for (int64_t e = e0; e < e0 + n_tail; ++e) {
            f32x4 pv = {p[e], 0.f, 0.f, 0.f}, mv = {m[e], 0.f, 0.f, 0.f}, vv = {v[e], 0.f, 0.f, 0.f};
            const f32x4 gv = {IO<DT_G>::load1(g, e) * grad_scale, 0.f, 0.f, 0.f};
            if constexpr (GROUPS == ADAM_NO_GROUPS) {
                // One call with a select between a local's address and null: the local lives in scratch, 32 bytes per lane, and the
                // launch WITH that scratch is the faster one.  Measured at bert-base (profiles/adam_one_body.md): the two-call form
                // below makes adam_kernel scratch-free and 0.05 - 0.08 % slower in every round; a cap on its waves instead helps or
                // hurts by box and by entry point.
                f32x4 vm4 = {vmax ? vmax[e] : 0.f, 0.f, 0.f, 0.f};          // (16-byte aligned: adam_update4 reads it as one vector)
                adam_update4<DEC>(pv, gv, mv, vv, vmax ? reinterpret_cast<float*>(&vm4) : nullptr, lr1, b1, b2, eps, wd1, keep1, bc1, bc2_sqrt);
                if (vmax) vmax[e] = vm4.x;
            } else if (vmax) {                                              // two calls: a pointer that is not a select of a local's
                f32x4 vm4 = {vmax[e], 0.f, 0.f, 0.f};                       // address and null keeps vm4 in registers (no scratch)
                adam_update4<DEC>(pv, gv, mv, vv, reinterpret_cast<float*>(&vm4), lr1, b1, b2, eps, wd1, keep1, bc1, bc2_sqrt);
                vmax[e] = vm4.x;
            } else {
                adam_update4<DEC>(pv, gv, mv, vv, nullptr, lr1, b1, b2, eps, wd1, keep1, bc1, bc2_sqrt);
            }
            p[e] = pv.x; m[e] = mv.x; v[e] = vv.x;
            if (shadow) IO<KVQ_BF16>::store1(shadow, e, pv.x);
        }
    }
}

template <int DT_G>
__global__ __launch_bounds__(256) void adam_kernel(
    float* __restrict__ p, const void* __restrict__ g, float* __restrict__ m, float* __restrict__ v, float* __restrict__ vmax,
    unsigned short* __restrict__ shadow, int64_t n4, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt,
    float grad_scale, const float* __restrict__ hyper, int n_tail, AdamFp8 f8, const GradGuard* __restrict__ guard) {
    adam_body<DT_G, ADAM_NO_GROUPS, false, true>(p, g, m, v, vmax, shadow, n4, n_tail, lr, b1, b2, eps, wd, bc1, bc2_sqrt, grad_scale, hyper, guard, f8,
                                                 nullptr, 0, nullptr, nullptr, 0);
}

// Parameter groups (kvq_adam_step_grouped*).  At most 4 waves per SIMD: measured at bert-base (profiles/adam_groups.md), this stream
// of seven 16-byte loads per thread runs SLOWER with more waves in flight -- 1.1 - 1.3 % behind adam_kernel at 6 waves, 0.7 - 0.8 %
// at 5, level with it at 4.
template <int DT_G, bool TABLE, bool DEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 4))) void adam_group_kernel(
    float* __restrict__ p, const void* __restrict__ g, float* __restrict__ m, float* __restrict__ v, float* __restrict__ vmax,
    unsigned short* __restrict__ shadow, int64_t n4, float b1, float b2, float eps, float wd_all, float grad_scale,
    const float* __restrict__ hyper, int n_tail, const unsigned char* __restrict__ bgroup, int64_t e_base,
    const float* __restrict__ g_scale, const float* __restrict__ g_wd, int n_groups, const GradGuard* __restrict__ guard) {
    adam_body<DT_G, TABLE ? ADAM_GROUP_TABLE : ADAM_ONE_GROUP, DEC, false>(p, g, m, v, vmax, shadow, n4, n_tail, 0.f, b1, b2, eps, wd_all, 1.f, 1.f, grad_scale,
                                                                          hyper, guard, AdamFp8{}, bgroup, e_base, g_scale, g_wd, n_groups);
}

// ---------------------------------------------------------------------------------------------------------------
// Device-resident step state: what changes from one training step to the next (step count -> dropout seed offset, learning
// rate after the MultiStepLR milestones, Adam bias corrections) lives in 24 bytes of HBM and is advanced by a one-thread kernel,
// so that a whole step captured in a hipGraph replays without any host-side argument patching.
// ---------------------------------------------------------------------------------------------------------------
struct StepState {
    unsigned long long step;   // optimiser steps completed; dropout kernels add it to their seed
    float lr, bc1, bc2s, pad;  // for the step being applied: lr after milestones, 1 - beta1^t, sqrt(1 - beta2^t)
};
struct Milestones {
    long long at[8];
    int n;
};

// step += 1 and the fields of that step t (1-based): lr = lr0 * gamma^k * warm * dec in double, rounded to f32 once, and the bias
// corrections.  warm: a linear warm-up over the first W steps; dec: a linear / cosine decay to r * lr0 at step T.  W = 0 and kind 0
// (kvq_step_state_advance) give the factor 1.0, which multiplies exactly: the bits of a state without a schedule.
__global__ void step_state_advance_sched_kernel(StepState* st, float lr0, float gamma, Milestones ms, float beta1, float beta2,
                                                long long W, int kind, long long T, float min_ratio) {
    const unsigned long long t = st->step + 1;                              // the step now being applied
    const double warm = (W > 0 && (long long)t < W) ? (double)t / (double)W : 1.0;
    double dec = 1.0;
    if (kind != 0) {
        const double r = (double)min_ratio;
        double x = ((double)(long long)t - (double)W) / ((double)T - (double)W);
        x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);                            // past T the rate stays at r * lr0 * gamma^k
        dec = kind == 1 ? 1.0 - (1.0 - r) * x : r + (1.0 - r) * 0.5 * (1.0 + cos(3.14159265358979323846 * x));
    }
    int k = 0;
    for (int i = 0; i < ms.n; ++i) k += ((long long)(t - 1) >= ms.at[i]) ? 1 : 0;   // MultiStepLR ticked once per finished step
    double lr = lr0;
    for (int i = 0; i < k; ++i) lr *= (double)gamma;
    st->lr = (float)(lr * (warm * dec));
    st->bc1 = (float)(1.0 - pow((double)beta1, (double)t));
    st->bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)t));
    st->step = t;
}

}  // namespace kvq

using namespace kvq;

// Every Adam entry point: the checks they share, the grid, the step state's floats and the dispatch.  `who` names the family in the
// error texts; gr != nullptr: the grouped kernels (which need a step state and carry no fp8 mirror).
struct AdamGroupArgs {
    const uint8_t* block_group;
    int64_t first_element;
    const float *lr_scale, *wd;
    int n_groups, decoupled;
};

static int adam_launch(const char* who, float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n,
                       int grad_dtype, const void* step_state, float lr, float beta1, float beta2, float eps, float weight_decay, float bc1,
                       float bc2s, float grad_scale, const void* guard, void* stream, const AdamFp8& f8 = AdamFp8{},
                       const AdamGroupArgs* gr = nullptr) {
    KVQ_REQUIRE(p && g && m && v && n > 0 && (step_state || !gr), "%s: bad argument", who);
    KVQ_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)vmax | (uintptr_t)shadow_bf16) & 15) == 0,
                "%s: 16-byte aligned buffers required", who);
    KVQ_REQUIRE(((uintptr_t)guard & 7) == 0, "%s: 8-byte aligned guard state required", who);
    if (gr) {
        KVQ_REQUIRE(gr->n_groups >= 1 && gr->n_groups <= 16 && (gr->decoupled == 0 || gr->decoupled == 1),
                    "%s: 1 .. 16 groups, decoupled 0 or 1", who);
        KVQ_REQUIRE(gr->first_element >= 0 && gr->first_element % 16 == 0, "%s: first_element must be a multiple of 16", who);
    }
    const int64_t n4 = n / 4;
    const int n_tail = (int)(n - 4 * n4);
    const int64_t n8 = (n4 + 1) / 2;
    unsigned blocks = (unsigned)((n8 + 255) / 256 > 32768 ? 32768 : (n8 + 255) / 256);
    if (blocks == 0) blocks = 1;
    // lr, bc1, bc2s of the step state (StepState), or null: the values passed by value
    const float* hyper = step_state ? reinterpret_cast<const float*>(reinterpret_cast<const char*>(step_state) + 8) : nullptr;
    const GradGuard* gd = reinterpret_cast<const GradGuard*>(guard);
    unsigned short* shadow = reinterpret_cast<unsigned short*>(shadow_bf16);
    const dim3 grid(blocks), block(256);
    hipStream_t st = (hipStream_t)stream;
    // the instantiations by [gradient dtype: KVQ_F32, anything else bf16] and, grouped, [block table][decoupled]
#define KVQ_ADAM_GROUP_KERNELS(DT_G)                                                    \
    {{adam_group_kernel<DT_G, false, false>, adam_group_kernel<DT_G, false, true>},   \
     {adam_group_kernel<DT_G, true, false>, adam_group_kernel<DT_G, true, true>}}
    static constexpr decltype(&adam_kernel<KVQ_F32>) plain[2] = {adam_kernel<KVQ_F32>, adam_kernel<KVQ_BF16>};
    static constexpr decltype(&adam_group_kernel<KVQ_F32, false, false>) grouped[2][2][2] = {KVQ_ADAM_GROUP_KERNELS(KVQ_F32),
                                                                                             KVQ_ADAM_GROUP_KERNELS(KVQ_BF16)};
#undef KVQ_ADAM_GROUP_KERNELS
    const int dt = grad_dtype != KVQ_F32;
    if (!gr)
        hipLaunchKernelGGL(plain[dt], grid, block, 0, st, p, g, m, v, vmax, shadow, n4, lr, beta1, beta2, eps, weight_decay, bc1, bc2s,
                           grad_scale, hyper, n_tail, f8, gd);
    else
        hipLaunchKernelGGL(grouped[dt][gr->block_group != nullptr][gr->decoupled], grid, block, 0, st, p, g, m, v, vmax, shadow, n4, beta1,
                           beta2, eps, weight_decay, grad_scale, hyper, n_tail, gr->block_group, gr->first_element, gr->lr_scale, gr->wd,
                           gr->n_groups, gd);
    return check_launch(gr ? "adam_group_kernel" : "adam_kernel");
}

// the mirror arguments of the two _fp8 entry points
static int adam_fp8_args(const char* who, AdamFp8* f8, void* w8_mirror, const int* span_segment, const float* seg_scale,
                         const int64_t* seg_off, const int64_t* seg_n, int nseg, int64_t first_element, int64_t n) {
    KVQ_REQUIRE(w8_mirror && span_segment && seg_scale && seg_off && seg_n && nseg > 0, "%s: null fp8 argument", who);
    KVQ_REQUIRE(first_element >= 0 && first_element % 8 == 0 && n % 8 == 0 && ((uintptr_t)w8_mirror & 7) == 0,
                "%s: the range must start and end at multiples of 8 elements", who);
    *f8 = AdamFp8{(unsigned char*)w8_mirror, span_segment, seg_scale, seg_off, seg_n, nseg, first_element};
    return KVQ_OK;
}

int kvq_adam_step(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                  void* stream) {
    KVQ_REQUIRE(step >= 1, "kvq_adam_step: step >= 1");
    // in double and rounded once, as the step state's kernel does it: 1.0f - powf(beta2, step) loses 55 f32 ulps of bc2s at
    // beta2 = 0.999, step 2 (the power rounds to f32 next to 1 and the difference keeps that absolute error)
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    return adam_launch("kvq_adam_step", p, g, m, v, vmax, shadow_bf16, n, grad_dtype, nullptr, lr, beta1, beta2, eps, weight_decay, bc1, bc2s,
                       grad_scale, nullptr, stream);
}

int kvq_adam_step_dev(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                      const void* step_state, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                      void* stream) {
    KVQ_REQUIRE(step_state, "kvq_adam_step_dev: null step state");
    return adam_launch("kvq_adam_step", p, g, m, v, vmax, shadow_bf16, n, grad_dtype, step_state, 0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f,
                       grad_scale, nullptr, stream);
}

int kvq_adam_step_dev_fp8(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                          const void* step_state, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                          void* w8_mirror, const int* span_segment, const float* seg_scale, const int64_t* seg_off, const int64_t* seg_n,
                          int nseg, int64_t first_element, void* stream) {
    KVQ_REQUIRE(step_state && shadow_bf16, "kvq_adam_step_dev_fp8: step state and bf16 shadow required");
    AdamFp8 f8;
    if (int rc = adam_fp8_args("kvq_adam_step_dev_fp8", &f8, w8_mirror, span_segment, seg_scale, seg_off, seg_n, nseg, first_element, n)) return rc;
    return adam_launch("kvq_adam_step", p, g, m, v, vmax, shadow_bf16, n, grad_dtype, step_state, 0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f,
                       grad_scale, nullptr, stream, f8);
}

// the two entry points above behind a gradient guard (csrc/kvq_gradnorm.hip): scale = grad_scale * guard->coef, nothing stored on a skip
int kvq_adam_step_guarded(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                          const void* step_state, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                          const void* guard, void* stream) {
    KVQ_REQUIRE(step_state && guard, "kvq_adam_step_guarded: null step state or guard state");
    return adam_launch("kvq_adam_step", p, g, m, v, vmax, shadow_bf16, n, grad_dtype, step_state, 0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f,
                       grad_scale, guard, stream);
}

int kvq_adam_step_guarded_fp8(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                              const void* step_state, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                              void* w8_mirror, const int* span_segment, const float* seg_scale, const int64_t* seg_off,
                              const int64_t* seg_n, int nseg, int64_t first_element, const void* guard, void* stream) {
    KVQ_REQUIRE(step_state && shadow_bf16 && guard, "kvq_adam_step_guarded_fp8: step state, bf16 shadow and guard state required");
    AdamFp8 f8;
    if (int rc = adam_fp8_args("kvq_adam_step_guarded_fp8", &f8, w8_mirror, span_segment, seg_scale, seg_off, seg_n, nseg, first_element, n)) return rc;
    return adam_launch("kvq_adam_step", p, g, m, v, vmax, shadow_bf16, n, grad_dtype, step_state, 0.f, beta1, beta2, eps, weight_decay, 1.f, 1.f,
                       grad_scale, guard, stream, f8);
}

// parameter groups (no fp8 mirror; the guard is optional)
int kvq_adam_step_grouped(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                          const void* step_state, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                          const uint8_t* block_group, int64_t first_element, const float* group_lr_scale, const float* group_wd,
                          int n_groups, int decoupled, void* stream) {
    const AdamGroupArgs gr = {block_group, first_element, group_lr_scale, group_wd, n_groups, decoupled};
    return adam_launch("kvq_adam_step_grouped", p, g, m, v, vmax, shadow_bf16, n, grad_dtype, step_state, 0.f, beta1, beta2, eps, weight_decay,
                       1.f, 1.f, grad_scale, nullptr, stream, AdamFp8{}, &gr);
}

int kvq_adam_step_grouped_guarded(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                                  const void* step_state, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                  const uint8_t* block_group, int64_t first_element, const float* group_lr_scale, const float* group_wd,
                                  int n_groups, int decoupled, const void* guard, void* stream) {
    KVQ_REQUIRE(guard, "kvq_adam_step_grouped_guarded: null guard state");
    const AdamGroupArgs gr = {block_group, first_element, group_lr_scale, group_wd, n_groups, decoupled};
    return adam_launch("kvq_adam_step_grouped", p, g, m, v, vmax, shadow_bf16, n, grad_dtype, step_state, 0.f, beta1, beta2, eps, weight_decay,
                       1.f, 1.f, grad_scale, guard, stream, AdamFp8{}, &gr);
}

// both step-state entry points: `who` names the caller in the text of the shared check
static int step_state_launch(const char* who, void* step_state, float lr0, float gamma, const int64_t* milestones, int n_milestones,
                             float beta1, float beta2, int64_t warmup_steps, int decay_kind, int64_t total_steps, float min_ratio,
                             void* stream) {
    KVQ_REQUIRE(step_state && n_milestones >= 0 && n_milestones <= 8 && (n_milestones == 0 || milestones),
                "%s: bad argument (at most 8 milestones)", who);
    KVQ_REQUIRE(warmup_steps >= 0 && decay_kind >= 0 && decay_kind <= 2 && (decay_kind == 0 || total_steps > warmup_steps) &&
                    min_ratio >= 0.f && min_ratio <= 1.f,
                "%s: warmup_steps >= 0, decay_kind 0 / 1 / 2, total_steps > warmup_steps, min_ratio in [0, 1]", who);
    Milestones ms = {};
    ms.n = n_milestones;
    for (int i = 0; i < n_milestones; ++i) ms.at[i] = milestones[i];
    hipLaunchKernelGGL(step_state_advance_sched_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (StepState*)step_state, lr0, gamma, ms,
                       beta1, beta2, (long long)warmup_steps, decay_kind, (long long)total_steps, min_ratio);
    return check_launch("step_state_advance_sched_kernel");
}

int kvq_step_state_advance_sched(void* step_state, float lr0, float gamma, const int64_t* milestones, int n_milestones, float beta1,
                                 float beta2, int64_t warmup_steps, int decay_kind, int64_t total_steps, float min_ratio, void* stream) {
    return step_state_launch("kvq_step_state_advance_sched", step_state, lr0, gamma, milestones, n_milestones, beta1, beta2, warmup_steps,
                             decay_kind, total_steps, min_ratio, stream);
}

// the neutral schedule: the factor 1.0
int kvq_step_state_advance(void* step_state, float lr0, float gamma, const int64_t* milestones, int n_milestones, float beta1,
                           float beta2, void* stream) {
    return step_state_launch("kvq_step_state_advance", step_state, lr0, gamma, milestones, n_milestones, beta1, beta2, 0, 0, 0, 0.f, stream);
}
