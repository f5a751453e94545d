// kvq_latent.hip -- the latent analyses' device side on gfx950: per-group sums of encoder outputs, the shift of a latent along
// the difference of two group means, and the codebook gather without distances.
//
// Boundary mirrored: analyses/latent_arithmetics/latent_arithmetics_Bagon.py:77-139 keeps every encoder output of three groups of
// sentences on the host, averages two of them and adds the difference to the third before decoding;
// analyses/latent_traversals/latent_traversals_Shelgon_latent_classes.py:113-161 overwrites code indices and looks the rows up.
// Here the sums stay on the device in f64 (table[G, S, H] += ..., no limit on the number of batches), the shift reads them there,
// and the lookup writes the codebook rows straight into the decoder's cross-attention source.
//
// All three are streaming kernels (a few bytes of arithmetic per byte moved): a lane moves 16 bytes of activations per access
// where the rows allow it (base and row stride 16-byte aligned), the columns past the last whole 16-byte piece -- or every
// column of rows that are not aligned -- go one element per lane.  None of them is on the training step.
#include "kvq_common.h"

namespace kvq {

constexpr int LAT_THREADS = 256;
constexpr int LAT_MAX_RUNS = 256;     // slabs of one kvq_latent_group_sum call at most: what the second launch reads per cell
constexpr int LAT_MIN_RUN = 8;        // sentences per workgroup at least (the floor kvq_attn_probs measured for its slab pass)

// elements of one 16-byte piece
template <int DT>
struct Piece {
    static constexpr int n = 16 / IO<DT>::bytes;
};

template <int DT>
__device__ __forceinline__ void piece_decode(const uint4 r, float (&v)[Piece<DT>::n]);
template <>
__device__ __forceinline__ void piece_decode<KVQ_F32>(const uint4 r, float (&v)[4]) {
    v[0] = __uint_as_float(r.x); v[1] = __uint_as_float(r.y); v[2] = __uint_as_float(r.z); v[3] = __uint_as_float(r.w);
}
template <>
__device__ __forceinline__ void piece_decode<KVQ_BF16>(const uint4 r, float (&v)[8]) {
    v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
    v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
    v[4] = __uint_as_float(r.z << 16); v[5] = __uint_as_float(r.z & 0xffff0000u);
    v[6] = __uint_as_float(r.w << 16); v[7] = __uint_as_float(r.w & 0xffff0000u);
}
template <int DT>
__device__ __forceinline__ uint4 piece_encode(const float (&v)[Piece<DT>::n]);
template <>
__device__ __forceinline__ uint4 piece_encode<KVQ_F32>(const float (&v)[4]) {
    return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
}
template <>
__device__ __forceinline__ uint4 piece_encode<KVQ_BF16>(const float (&v)[8]) {
    unsigned w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) w[u] = (unsigned)f32_to_bf16(v[2 * u]) | ((unsigned)f32_to_bf16(v[2 * u + 1]) << 16);
    return make_uint4(w[0], w[1], w[2], w[3]);
}
template <int DT>
__device__ __forceinline__ uint4 piece_load(const void* base, size_t off) {
    return *reinterpret_cast<const uint4*>(reinterpret_cast<const typename IO<DT>::elem*>(base) + off);
}
template <int DT>
__device__ __forceinline__ void piece_store(void* base, size_t off, const uint4 r) {
    *reinterpret_cast<uint4*>(reinterpret_cast<typename IO<DT>::elem*>(base) + off) = r;
}

// n consecutive doubles; two per access where the address is 16-byte aligned (n is even then: 4 or 8)
template <int N>
__device__ __forceinline__ void f64_load(const double* p, double (&v)[N]) {
    if (N > 1 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int u = 0; u < N / 2; ++u) {
            const double2 d = reinterpret_cast<const double2*>(p)[u];
            v[2 * u] = d.x; v[2 * u + 1] = d.y;
        }
    } else {
#pragma unroll
        for (int u = 0; u < N; ++u) v[u] = p[u];
    }
}
template <int N>
__device__ __forceinline__ void f64_store(double* p, const double (&v)[N]) {
    if (N > 1 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int u = 0; u < N / 2; ++u) reinterpret_cast<double2*>(p)[u] = make_double2(v[2 * u], v[2 * u + 1]);
    } else {
#pragma unroll
        for (int u = 0; u < N; ++u) p[u] = v[u];
    }
}

// A row of W columns as work items: `pieces` whole 16-byte pieces first, then the remaining columns one by one.
struct RowItems {
    int pieces;       // 0 when the rows are not 16-byte aligned
    int per_row;      // pieces + (W - pieces * n)
};
static RowItems row_items(int W, int n, bool aligned) {
    RowItems r;
    r.pieces = aligned ? W / n : 0;
    r.per_row = r.pieces + (W - r.pieces * n);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------
// kvq_latent_group_sum.  Workgroup (run, span): sentences [run * R, min(B, run * R + R)), 256 items of the [S, H] plane.  For each
// group in turn it adds the run's sentences of that group in ascending order in f64 registers and leaves them in
// slab[run][g][S * H] (zeros when the run holds none), so every cell of every slab is written by exactly one lane.  The workgroups
// of span 0 also count their run's sentences per group (integer atomics: exact, order-free) and the labels outside [-1, G).
// group_slabs_kernel then adds the slabs of a cell in ascending run order into the caller's table.
// ---------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(LAT_THREADS) void group_sum_kernel(const void* __restrict__ x, int64_t ldx, const int32_t* __restrict__ group,
                                                                int64_t B, int S, int H, int G, int run_len, RowItems it, int64_t slab_ld,
                                                                double* __restrict__ slab, unsigned long long* __restrict__ count,
                                                                uint32_t* __restrict__ n_bad) {
    constexpr int n = Piece<DT>::n;
    const int64_t run = blockIdx.y;
    const int64_t b0 = run * run_len, b1 = b0 + run_len < B ? b0 + run_len : B;
    if (blockIdx.x == 0) {
        for (int64_t b = b0 + threadIdx.x; b < b1; b += LAT_THREADS) {
            const int32_t g = group[b];
            if (g == -1) continue;
            if (g < -1 || g >= G) { if (n_bad) atomicAdd(n_bad, 1u); }
            else atomicAdd(&count[g], 1ull);
        }
    }
    const int64_t item = (int64_t)blockIdx.x * LAT_THREADS + threadIdx.x;
    if (item >= (int64_t)S * it.per_row) return;
    const int s = (int)(item / it.per_row), j = (int)(item % it.per_row);
    const bool piece = j < it.pieces;
    const int h = piece ? j * n : it.pieces * n + (j - it.pieces);
    for (int g = 0; g < G; ++g) {
        double acc[n];
#pragma unroll
        for (int u = 0; u < n; ++u) acc[u] = 0.0;
        for (int64_t b = b0; b < b1; ++b) {
            if (group[b] != g) continue;                     // (uniform over the workgroup)
            const size_t off = (size_t)(b * S + s) * ldx + h;
            if (piece) {
                float v[n];
                piece_decode<DT>(piece_load<DT>(x, off), v);
#pragma unroll
                for (int u = 0; u < n; ++u) acc[u] += (double)v[u];
            } else {
                acc[0] += (double)IO<DT>::load1(x, off);
            }
        }
        double* dst = slab + (run * G + g) * slab_ld + (int64_t)s * H + h;
        if (piece) f64_store<n>(dst, acc);
        else dst[0] = acc[0];
    }
}

// table[c] += slab[0][c] + slab[1][c] + ... in that order; two cells per lane (slab_ld is even, the bases are 16-byte aligned)
__global__ __launch_bounds__(LAT_THREADS) void group_slabs_kernel(const double* __restrict__ slab, int runs, int G, int64_t cells,
                                                                  int64_t slab_ld, double* __restrict__ table) {
    const int64_t pair = (int64_t)blockIdx.x * LAT_THREADS + threadIdx.x;
    const int g = blockIdx.y;
    const int64_t c = 2 * pair;
    if (c >= cells) return;
    double* t = table + (int64_t)g * cells + c;
    if (c + 1 < cells && ((uintptr_t)t & 15) == 0) {
        double2 a = *reinterpret_cast<double2*>(t);
        for (int r = 0; r < runs; ++r) {
            const double2 d = *reinterpret_cast<const double2*>(slab + ((int64_t)r * G + g) * slab_ld + c);
            a.x += d.x; a.y += d.y;
        }
        *reinterpret_cast<double2*>(t) = a;
    } else {
        const int m = c + 1 < cells ? 2 : 1;
        for (int u = 0; u < m; ++u) {
            double a = t[u];
            for (int r = 0; r < runs; ++r) a += slab[((int64_t)r * G + g) * slab_ld + c + u];
            t[u] = a;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// kvq_latent_shift.  One item = one 16-byte piece (or one trailing column) of one (b, s) row; each lane reads its elements before it
// writes them, so out may be x.  f64 throughout: d = table[g1] / count[g1] - table[g0] / count[g0], r = x + alpha * d, rounded to
// f32 and then to the io dtype.  -ffp-contract=off (build.sh): the product and the sum round separately, as written.
// ---------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(LAT_THREADS) void latent_shift_kernel(const void* x, int64_t ldx, const double* __restrict__ table,
                                                                   const int64_t* __restrict__ count, int g1, int g0, double alpha,
                                                                   const int8_t* __restrict__ sel, int64_t rows, int S, int H, RowItems it,
                                                                   void* out, int64_t ldo) {
    constexpr int n = Piece<DT>::n;
    const int64_t item = (int64_t)blockIdx.x * LAT_THREADS + threadIdx.x;
    if (item >= rows * it.per_row) return;
    const int64_t row = item / it.per_row;
    const int j = (int)(item % it.per_row);
    const int s = (int)(row % S);
    const bool piece = j < it.pieces;
    const int h = piece ? j * n : it.pieces * n + (j - it.pieces);
    const int64_t c1 = count[g1], c0 = count[g0];
    const bool on = (sel == nullptr || sel[row] != 0) && c1 > 0 && c0 > 0;       // an empty group: no shift
    const size_t xo = (size_t)row * ldx + h, oo = (size_t)row * ldo + h;
    const double* t1 = table + ((int64_t)g1 * S + s) * H + h;
    const double* t0 = table + ((int64_t)g0 * S + s) * H + h;
    const double n1 = (double)c1, n0 = (double)c0;
    if (piece) {
        const uint4 raw = piece_load<DT>(x, xo);
        if (!on) {
            if (out != x) piece_store<DT>(out, oo, raw);
            return;
        }
        float v[n];
        double a[n], b[n];
        piece_decode<DT>(raw, v);
        f64_load<n>(t1, a);
        f64_load<n>(t0, b);
#pragma unroll
        for (int u = 0; u < n; ++u) {
            const double d = a[u] / n1 - b[u] / n0;
            const double p = alpha * d;
            v[u] = (float)((double)v[u] + p);
        }
        piece_store<DT>(out, oo, piece_encode<DT>(v));
    } else {
        typedef typename IO<DT>::elem E;
        const E raw = reinterpret_cast<const E*>(x)[xo];
        if (!on) {
            if (out != x) reinterpret_cast<E*>(out)[oo] = raw;
            return;
        }
        const double d = t1[0] / n1 - t0[0] / n0;
        const double p = alpha * d;
        IO<DT>::store1(out, oo, (float)((double)IO<DT>::load1(x, xo) + p));
    }
}

// ---------------------------------------------------------------------------------------------------------------
// kvq_vq_lookup.  One item = one 16-byte piece of OUTPUT (4 f32 or 8 bf16 columns of factor g's slice of token n) or one trailing
// column.  An index outside [0, K) leaves zeros and is counted once per (n, g).
// ---------------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(LAT_THREADS) void vq_lookup_kernel(const int64_t* __restrict__ idx, const float* __restrict__ E, int64_t N, int K,
                                                                int Dg, int G, RowItems it, void* __restrict__ out, int64_t ldo,
                                                                uint32_t* __restrict__ n_bad) {
    constexpr int n = Piece<DT>::n;
    const int64_t item = (int64_t)blockIdx.x * LAT_THREADS + threadIdx.x;
    if (item >= N * G * it.per_row) return;
    const int64_t ng = item / it.per_row;
    const int j = (int)(item % it.per_row);
    const int64_t tok = ng / G;
    const int g = (int)(ng % G);
    const bool piece = j < it.pieces;
    const int d = piece ? j * n : it.pieces * n + (j - it.pieces);
    const int64_t k = idx[ng];
    const bool ok = k >= 0 && k < K;
    if (!ok && j == 0 && n_bad) atomicAdd(n_bad, 1u);
    const float* e = E + ((int64_t)g * K + (ok ? k : 0)) * Dg + d;
    const size_t oo = (size_t)tok * ldo + (size_t)g * Dg + d;
    if (piece) {
        float v[n];
#pragma unroll
        for (int u = 0; u < n / 4; ++u) {
            const f32x4 q = ok ? *reinterpret_cast<const f32x4*>(e + 4 * u) : f32x4{0.f, 0.f, 0.f, 0.f};
            v[4 * u] = q.x; v[4 * u + 1] = q.y; v[4 * u + 2] = q.z; v[4 * u + 3] = q.w;
        }
        piece_store<DT>(out, oo, piece_encode<DT>(v));
    } else {
        IO<DT>::store1(out, oo, ok ? e[0] : 0.f);
    }
}

static int latent_run_len(int64_t B) {
    const int64_t r = (B + LAT_MAX_RUNS - 1) / LAT_MAX_RUNS;
    return r < LAT_MIN_RUN ? LAT_MIN_RUN : (int)r;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace kvq

using namespace kvq;

#define LATENT_DT(io_dtype, CALL_F32, CALL_BF16) \
    do {                                         \
        if ((io_dtype) == KVQ_F32) { CALL_F32; } \
        else { CALL_BF16; }                      \
    } while (0)

extern "C" {

size_t kvq_latent_group_sum_workspace_bytes(int64_t B, int S, int H, int G) {
    if (B <= 0 || S <= 0 || H <= 0 || G <= 0) return 0;
    const int R = latent_run_len(B);
    const size_t runs = (size_t)((B + R - 1) / R);
    const size_t cells = (size_t)S * H;
    return align_up(runs * G * (cells + (cells & 1)) * sizeof(double), 256);
}

int kvq_latent_group_sum(const void* x, int64_t ldx, const int32_t* group, int64_t B, int S, int H, int G, int io_dtype, double* table,
                         int64_t* count, uint32_t* n_bad, void* ws, size_t ws_bytes, void* stream) {
    KVQ_REQUIRE(B >= 0 && S >= 1 && H >= 1 && G >= 1, "kvq_latent_group_sum: B >= 0, S, H, G >= 1 required (B=%lld S=%d H=%d G=%d)",
                (long long)B, S, H, G);
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "kvq_latent_group_sum: io_dtype must be KVQ_F32 or KVQ_BF16");
    KVQ_REQUIRE(G <= 65535 && (int64_t)S * H < (int64_t)1 << 31, "kvq_latent_group_sum: G <= 65535 and S * H < 2^31 required");
    if (B == 0) return KVQ_OK;
    KVQ_REQUIRE(x && group && table && count, "kvq_latent_group_sum: null pointer argument");
    KVQ_REQUIRE(ldx >= H, "kvq_latent_group_sum: row stride %lld below H = %d", (long long)ldx, H);
    KVQ_REQUIRE(aligned16(table), "kvq_latent_group_sum: table must be 16-byte aligned");
    if (!(ws && ws_bytes >= kvq_latent_group_sum_workspace_bytes(B, S, H, G) && aligned16(ws)))
        return fail(KVQ_E_WORKSPACE, "kvq_latent_group_sum: needs a 16-byte aligned workspace of kvq_latent_group_sum_workspace_bytes(B, S, H, G) bytes");
    const int R = latent_run_len(B);
    const int runs = (int)((B + R - 1) / R);
    const int64_t cells = (int64_t)S * H, slab_ld = cells + (cells & 1);
    const int n = io_dtype == KVQ_F32 ? 4 : 8;
    const RowItems it = row_items(H, n, aligned16(x) && ldx % n == 0);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(((int64_t)S * it.per_row + LAT_THREADS - 1) / LAT_THREADS), (unsigned)runs);
    LATENT_DT(io_dtype,
              hipLaunchKernelGGL(group_sum_kernel<KVQ_F32>, grid, dim3(LAT_THREADS), 0, st, x, ldx, group, B, S, H, G, R, it, slab_ld,
                                 (double*)ws, (unsigned long long*)count, n_bad),
              hipLaunchKernelGGL(group_sum_kernel<KVQ_BF16>, grid, dim3(LAT_THREADS), 0, st, x, ldx, group, B, S, H, G, R, it, slab_ld,
                                 (double*)ws, (unsigned long long*)count, n_bad));
    int rc = check_launch("group_sum_kernel");
    if (rc) return rc;
    const dim3 grid2((unsigned)(((cells + 1) / 2 + LAT_THREADS - 1) / LAT_THREADS), (unsigned)G);
    hipLaunchKernelGGL(group_slabs_kernel, grid2, dim3(LAT_THREADS), 0, st, (const double*)ws, runs, G, cells, slab_ld, table);
    return check_launch("group_slabs_kernel");
}

int kvq_latent_shift(const void* x, int64_t ldx, const double* table, const int64_t* count, int g1, int g0, double alpha,
                     const int8_t* sel, int64_t B, int S, int H, int G, int io_dtype, void* out, int64_t ldo, void* stream) {
    KVQ_REQUIRE(B >= 0 && S >= 1 && H >= 1 && G >= 1, "kvq_latent_shift: B >= 0, S, H, G >= 1 required (B=%lld S=%d H=%d G=%d)",
                (long long)B, S, H, G);
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "kvq_latent_shift: io_dtype must be KVQ_F32 or KVQ_BF16");
    KVQ_REQUIRE(g1 >= 0 && g1 < G && g0 >= 0 && g0 < G, "kvq_latent_shift: groups %d, %d outside [0, %d)", g1, g0, G);
    if (B == 0) return KVQ_OK;
    KVQ_REQUIRE(x && table && count && out, "kvq_latent_shift: null pointer argument");
    KVQ_REQUIRE(ldx >= H && ldo >= H, "kvq_latent_shift: row strides %lld, %lld below H = %d", (long long)ldx, (long long)ldo, H);
    const int n = io_dtype == KVQ_F32 ? 4 : 8;
    const RowItems it = row_items(H, n, aligned16(x) && aligned16(out) && ldx % n == 0 && ldo % n == 0);
    const int64_t rows = B * S;
    const int64_t blocks = (rows * it.per_row + LAT_THREADS - 1) / LAT_THREADS;
    KVQ_REQUIRE(blocks < (int64_t)1 << 31, "kvq_latent_shift: %lld workgroups do not fit one launch", (long long)blocks);
    hipStream_t st = (hipStream_t)stream;
    LATENT_DT(io_dtype,
              hipLaunchKernelGGL(latent_shift_kernel<KVQ_F32>, dim3((unsigned)blocks), dim3(LAT_THREADS), 0, st, x, ldx, table, count, g1, g0,
                                 alpha, sel, rows, S, H, it, out, ldo),
              hipLaunchKernelGGL(latent_shift_kernel<KVQ_BF16>, dim3((unsigned)blocks), dim3(LAT_THREADS), 0, st, x, ldx, table, count, g1, g0,
                                 alpha, sel, rows, S, H, it, out, ldo));
    return check_launch("latent_shift_kernel");
}

int kvq_vq_lookup(const int64_t* idx, const float* E, int64_t N, int K, int Dg, int G, int io_dtype, void* out, int64_t ldo,
                  uint32_t* n_bad, void* stream) {
    KVQ_REQUIRE(N >= 0 && K >= 1 && Dg >= 1 && G >= 1, "kvq_vq_lookup: N >= 0, K, Dg, G >= 1 required (N=%lld K=%d Dg=%d G=%d)",
                (long long)N, K, Dg, G);
    KVQ_REQUIRE(io_dtype == KVQ_F32 || io_dtype == KVQ_BF16, "kvq_vq_lookup: io_dtype must be KVQ_F32 or KVQ_BF16");
    if (N == 0) return KVQ_OK;
    KVQ_REQUIRE(idx && E && out, "kvq_vq_lookup: null pointer argument");
    KVQ_REQUIRE(ldo >= (int64_t)G * Dg, "kvq_vq_lookup: row stride %lld below G * Dg = %lld", (long long)ldo, (long long)G * Dg);
    const int n = io_dtype == KVQ_F32 ? 4 : 8;
    // a piece starts at column g * Dg + j * n of a row: 16-byte aligned in the output when rows and slices are, and in the codebook
    // (f32 rows of Dg columns) when Dg is a multiple of 4
    const RowItems it = row_items(Dg, n, aligned16(out) && aligned16(E) && ldo % n == 0 && Dg % 4 == 0 && (G == 1 || Dg % n == 0));
    const int64_t blocks = (N * G * it.per_row + LAT_THREADS - 1) / LAT_THREADS;
    KVQ_REQUIRE(blocks < (int64_t)1 << 31, "kvq_vq_lookup: %lld workgroups do not fit one launch", (long long)blocks);
    hipStream_t st = (hipStream_t)stream;
    LATENT_DT(io_dtype,
              hipLaunchKernelGGL(vq_lookup_kernel<KVQ_F32>, dim3((unsigned)blocks), dim3(LAT_THREADS), 0, st, idx, E, N, K, Dg, G, it, out, ldo, n_bad),
              hipLaunchKernelGGL(vq_lookup_kernel<KVQ_BF16>, dim3((unsigned)blocks), dim3(LAT_THREADS), 0, st, idx, E, N, K, Dg, G, it, out, ldo, n_bad));
    return check_launch("vq_lookup_kernel");
}

}  // extern "C"
