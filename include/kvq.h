/*
 * kvq.h -- C ABI of libkvq.so: the MI355X (gfx950) implementation of the Kindergarten-VQ-VAE
 * Shelgon/Bagon training hot path.
 *
 * The reference has no FFI (it is pure Python on ATen); the boundary this library sits
 * behind is the reference's nn.Module / function surface.  Each entry point below names the reference
 * lines it replaces.  The Python host (kindergarten-vq-vae_amd/kvq/_ffi.py) binds exactly these symbols
 * with ctypes and hands over raw device pointers (tensor.data_ptr()) and the current HIP stream.
 *
 * Conventions
 *   - every function returns 0 on success, a negative KVQ_E_* code on failure; the message of the last
 *     failure on the calling thread is kvq_last_error().  Nothing throws, nothing is allocated or freed
 *     on behalf of the caller, no host synchronisation happens: all work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream).  All entry points are hipGraph-capturable and enqueue
 *     KERNELS only: no stream memset, no memcpy (a memset captured as a graph node was observed in round 4 not to keep its
 *     stream order ahead of the next kernel node, profiles/r04_fp8.md; kvq_graph_census lets a caller check what it captured).
 *   - all pointers are DEVICE pointers unless the name ends in _host.
 *   - tensors are dense row-major; "io dtype" is the storage type of activations (z, z_q, g_zq, g_z, logits):
 *     KVQ_F32 or KVQ_BF16.  The codebook E and its gradient are always f32, all arithmetic is f32
 *     (exact f32 MFMA for the distance contraction) whatever the io dtype.
 *   - G = number of independent codebooks ("factors").  G = 1 is the reference.
 *     Layouts: z[G,N,D], E[G,K,D], idx[G,N], loss[G], perplexity[G], counts[G,K].
 *
 * Numerics contract of the VQ forward ("kvq order v1", restated on the CPU in oracle/vq_oracle.c):
 *   dot(n,k)  = one f32 fmaf chain over j, visiting each group of 8 consecutive j in the order
 *               0,4,1,5,2,6,3,7 (the k-walk of v_mfma_f32_32x32x2_f32 fed by 16-byte fragments)
 *   sq(x)     = fl(p0 + p1), p_h = fmaf chain of x[j]^2 over increasing j with (j mod 8)/4 == h
 *   d(n,k)    = fl( fl(sq(z_n) + sq(e_k)) - fl(2*dot(n,k)) )            [VectorQuantizer.py:59-61]
 *   idx(n)    = first k attaining the minimum (NaN counts as smallest, as torch.argmin) [:65]
 *   z_q(n)    = fl( z_n + fl(e_idx - z_n) )                              [:72,:80]
 *   loss      = fl(m + fl(beta*m)),  m = (sum of fl(e_idx - z_n)^2 in f64) / (N*D)     [:76-77]
 *   perplexity= exp(-sum_k p_k*log(p_k + 1e-10)),  p_k = count_k / N  (f32)            [:84-85]
 */
#ifndef KVQ_H
#define KVQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KVQ_VERSION 100 /* 0.1.0 */

/* io dtypes */
#define KVQ_F32 0
#define KVQ_BF16 1

/* error codes */
#define KVQ_OK 0
#define KVQ_E_INVALID (-1)   /* bad argument (null pointer, non-positive size, unsupported dtype) */
#define KVQ_E_WORKSPACE (-2) /* workspace too small / missing */
#define KVQ_E_LAUNCH (-3)    /* HIP reported a launch error */
#define KVQ_E_NODEVICE (-4)  /* no HIP device usable */

int kvq_version(void);
const char* kvq_last_error(void);

/* What a captured hipGraph consists of (host call, no stream): counts_host[KVQ_GRAPH_NODE_KINDS] = nodes of `graph` (a hipGraph_t)
 * by kind.  The TrainEngine's step graphs must hold kernel nodes only (tests/test_graph_nodes_gpu.py asserts it on the graphs
 * the benchmark replays); no reference counterpart. */
#define KVQ_GRAPH_NODE_KERNEL 0
#define KVQ_GRAPH_NODE_MEMSET 1
#define KVQ_GRAPH_NODE_MEMCPY 2
#define KVQ_GRAPH_NODE_EMPTY 3  /* joins of forked streams */
#define KVQ_GRAPH_NODE_EVENT 4  /* event record / wait nodes */
#define KVQ_GRAPH_NODE_OTHER 5
#define KVQ_GRAPH_NODE_KINDS 6
int kvq_graph_census(void* graph, int64_t* counts_host);

/* dst[rows_padded][row_bytes] = the first `rows` rows of src (row stride src_ld_bytes), then zero rows.  All sizes and both
 * buffers in multiples of 16 bytes.  Used for the operands of a weight-gradient product gy^T . x (autograd of every nn.Linear,
 * modeling_bert.py) whose token count is not a multiple of 64, the contraction depth of one MFMA k-tile: zero rows add nothing. */
int kvq_pad_rows(const void* src, int64_t rows, int64_t row_bytes, int64_t src_ld_bytes, void* dst, int64_t rows_padded, void* stream);

/* Number of compute units / name of the device the calling thread would launch on (diagnostics only). */
int kvq_device_info(int* cu_count, char* name, size_t name_len);

/* ------------------------------------------------------------------------------------------------
 * VectorQuantizer.forward  (models/shelgon3/VectorQuantizer.py:31-93)
 *
 *   z        [G,N,D] io dtype   encoder output, N = B*S tokens          (:52-55)
 *   E        [G,K,D] f32        codebook = embedding.weight             (:25)
 *   z_q      [G,N,D] io dtype   straight-through output value           (:72,:80)
 *   idx      [G,N]   int64      min_encoding_indices                    (:65,:90)
 *   loss     [G]     f32        codebook + commitment loss              (:76-77)
 *   perplexity [G]   f32                                                (:84-85)
 *   counts   [G,K]   f32        code usage histogram = sum(min_encodings,0); may be NULL
 *   ws                         scratch of kvq_vq_workspace_bytes(N,K,D,G) bytes, 256-byte aligned
 *
 * What runs per call on the fast path (D %% 32 == 0): a small kernel that resets the minima / histogram / arrival tickets, then ONE
 * kernel for everything of :55-85 -- the f32-MFMA distance / arg-min contraction (64-bit integer atomicMin per token); the
 * workgroup that delivers the LAST code block of a token block goes on to gather, straight-through, per-token loss terms and
 * histogram for those tokens, and the token block that finishes last of all turns the partials into loss / perplexity in a
 * fixed order (no float atomics: bitwise reproducible) -- plus, in kvq_vq_forward only, the re-layout of the codebook in
 * MFMA-fragment order.  kvq_vq_set_variant(0) splits the tail off again into an epilogue and a finalize kernel (rounds 1 - 4;
 * the A/B arm and the checker of the fused tail; per calling thread, the product path never changes it).  A caller that quantises with one codebook many times between its updates (a
 * training loop: one update per optimiser step) keeps that copy itself: kvq_vq_pack_codebook after every codebook update,
 * kvq_vq_forward_packed per step.  Other D: one generic kernel (one wave per token) + the same finalize.
 * min_encodings ([N,K] one-hot, :67-68) is not produced here: see kvq_vq_one_hot.
 */
size_t kvq_vq_workspace_bytes(int64_t N, int K, int D, int G);

int kvq_vq_forward(const void* z, const float* E, int64_t N, int K, int D, int G, int io_dtype, float beta,
                   void* z_q, int64_t* idx, float* loss, float* perplexity, float* counts,
                   void* ws, size_t ws_bytes, void* stream);
int kvq_vq_set_variant(int fused);
/* packed: kvq_vq_packed_bytes(K, D, G) bytes, 16-byte aligned, written by kvq_vq_pack_codebook from the SAME E (D %% 32 == 0). */
size_t kvq_vq_packed_bytes(int K, int D, int G);
int kvq_vq_pack_codebook(const float* E, int K, int D, int G, float* packed, void* stream);
int kvq_vq_forward_packed(const void* z, const float* E, const float* packed, int64_t N, int K, int D, int G, int io_dtype,
                          float beta, void* z_q, int64_t* idx, float* loss, float* perplexity, float* counts,
                          void* ws, size_t ws_bytes, void* stream);

/* Autograd of the above (implicit in the reference; closed form in SURVEY.md §8 row A8b):
 *   g_z  = g_zq - s*fl(e_idx - z),            s = g_loss * 2/(N*D)
 *   g_E[k] = beta*s * sum_{n: idx_n = k} fl(e_k - z_n)      (deterministic: ordered slab reduction, no atomics)
 *   g_zq   [G,N,D] io dtype  upstream gradient of z_q (may be NULL = zeros)
 *   g_loss [G]     f32       upstream gradient of loss, ON DEVICE (may be NULL = ones)
 *   g_z    [G,N,D] io dtype ; g_E [G,K,D] f32 (overwritten, not accumulated); either may be NULL to skip.
 */
int kvq_vq_backward(const void* z, const float* E, const int64_t* idx, const void* g_zq, const float* g_loss,
                    int64_t N, int K, int D, int G, int io_dtype, float beta,
                    void* g_z, float* g_E, void* ws, size_t ws_bytes, void* stream);

/* min_encodings = one_hot(idx) as f32 [N,K]  (VectorQuantizer.py:67-68).  Materialised only on request. */
int kvq_vq_one_hot(const int64_t* idx, int64_t N, int K, float* enc, void* stream);

/* Test hook: the f32 distance matrix d[N,K] exactly as the fused kernel sees it (fast MFMA path when
 * `use_mfma` != 0 and the shape allows, otherwise the generic path).  Not used by the product path. */
int kvq_vq_debug_distances(const void* z, const float* E, int64_t N, int K, int D, int io_dtype,
                           int use_mfma, float* d, void* stream);

/* Kernel timing hook for bench.py's roofline line.  While enabled, every kvq_vq_forward call brackets its FUSED
 * kernel (not the memset / finalize launches) with a pair of HIP events recorded on the call's stream.
 *   kvq_prof_enable(n) : n > 0 allocates a ring of n event pairs and starts recording; n == 0 stops and frees.
 *   kvq_prof_read(ms, max) : after the caller has synchronised the stream, writes up to `max` durations in
 *                            milliseconds (oldest first), clears the ring and returns how many were written. */
int kvq_prof_enable(int n_pairs);
int kvq_prof_read(float* ms_host, int max);

/* Clock probe (measurement aid of bench.py; no reference counterpart): every one of kvq_clock_probe_rows() single-wave workgroups
 * stores out[row] = {XCC id, s_memtime, s_memrealtime, HW_ID} (4 x uint64).  Two probes on one stream bracket a region: per XCD,
 * (memtime_1 - memtime_0) / (memrealtime_1 - memrealtime_0) x 100 MHz is the shader clock the chip held there (DVFS included);
 * the peaks of MI355X_MICROARCH.md are quoted at 2.4 GHz.  Product kernels carry no stamps. */
int kvq_clock_probe_rows(void);
int kvq_clock_probe(uint64_t* out, size_t out_bytes, void* stream);

/* Which path kvq_vq_forward takes for a shape: 1 = f32-MFMA LDS-tiled kernel, 0 = generic kernel. */
int kvq_vq_uses_mfma(int64_t N, int K, int D);

/* EMA codebook update (extension named by BASELINE.json north_star; NOT in the reference -> default off):
 *   n_k <- g*n_k + (1-g)*count_k ;  m_k <- g*m_k + (1-g)*sum_{idx_n=k} z_n ;
 *   E_k <- m_k / ((n_k + eps)/(sum n + K*eps) * sum n)
 *   ema_n [G,K] f32, ema_m [G,K,D] f32 and E are updated in place. */
int kvq_vq_ema_update(const void* z, const int64_t* idx, int64_t N, int K, int D, int G, int io_dtype,
                      float decay, float eps, float* ema_n, float* ema_m, float* E,
                      void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Reconstruction loss of step()  (models/shelgon3/Trainer.py:94-101)
 *
 *   kl_div(log_softmax(logits), one_hot(ids), "batchmean")  ==  mean_n( logsumexp(logits_n) - logits_n[ids_n] )
 *   recon_ids = argmax(softmax(logits)) == argmax(logits) (first maximum)
 *
 *   logits [N,V] io dtype ; target [N] int64 ; row_loss [N] f32 ; row_lse [N] f32 ; pred [N] int64
 *   loss [1] f32 = mean(row_loss) ; acc [1] f32 = mean(pred == target)  (common/metrics.py:18-30)
 * The [N,V] one-hot of the reference (1 GB at N=8192) is never built.
 * Logits of -inf are allowed off the target: they add 0 to the row's sum, row_lse stays finite and their gradient is exactly 0.
 * A row whose target logit is -inf has row_loss = +inf (and so has the mean).  +inf and NaN logits are not supported.
 */
int kvq_ce_forward(const void* logits, const int64_t* target, int64_t N, int V, int64_t ld, int io_dtype,
                   float* row_loss, float* row_lse, int64_t* pred, float* loss, float* acc, void* stream);

/* seq_acc's per-sentence result (common/metrics.py:32-36; consumed as stats_step["metric_acc_step_per_sentence"] by
 * models/bagon/Trainer.py:107,275): per_sentence[b] = mean over s of (pred[b,s] == target[b,s]); pred / target [B,S] int64 row-major
 * (pred = kvq_ce_forward's arg-max).  The per-batch value is kvq_ce_forward's `acc`. */
int kvq_seq_acc(const int64_t* pred, const int64_t* target, int64_t B, int S, float* per_sentence, void* stream);

/* The same results from the per-tile statistics of kvq_gemm_bf16_ce (below): stats [N][tiles][4] f32 = (max, sum exp(x - max),
 * first arg-max as int bits, unused) of row n over tile t's columns < V.  Reads ONE logit per row (the target's); the [N, V]
 * logits are not read again.  SURVEY.md §8(f) rank 1. */
int kvq_ce_forward_stats(const void* logits, const int64_t* target, int64_t N, int64_t ld, int io_dtype, const float* stats, int tiles,
                         float* row_loss, float* row_lse, int64_t* pred, float* loss, float* acc, void* stream);

/* g_logits[n,v] = g_loss/N * (softmax(logits_n)[v] - [v == target_n]); may alias logits (in place). */
int kvq_ce_backward(const void* logits, const int64_t* target, const float* row_lse, const float* g_loss,
                    int64_t N, int V, int64_t ld, int io_dtype, void* g_logits, void* stream);
/* kvq_ce_backward that also leaves bias_part [kvq_ce_bwd_partial_rows(N)][ld] f32 = partial column sums of g_logits (as stored):
 * the gradient of the LM-head output bias (modeling_bert.py:483-497), finished by kvq_reduce_batch -- no second pass over
 * the [N, V] gradient.  Needs ld %% 8 == 0 and 16-byte aligned buffers; columns V .. ld of g_logits and of the sums are 0. */
int64_t kvq_ce_bwd_partial_rows(int64_t N);
int kvq_ce_backward_bias(const void* logits, const int64_t* target, const float* row_lse, const float* g_loss, int64_t N,
                         int V, int64_t ld, int io_dtype, void* g_logits, float* bias_part, size_t part_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The same loss over the COUNTED rows only (F.cross_entropy's ignore_index).  Row n is IGNORED iff
 * target[n] == ignore_index, which may lie outside [0, V) (e.g. -100); every other row is counted and must have 0 <= target < V.
 *
 *   counted row : row_loss / row_lse / pred / gradient exactly as in the entry points above
 *   ignored row : row_loss = 0, row_lse = 0, pred = ignore_index, gradient row (padding columns included) = +0.  Nothing of its
 *                 logits row is read -- not by the forward (no load at x[target]), not by the backward, not even in place -- so NaN
 *                 or garbage there reaches no output.
 *   count [1] f32 = number of counted rows, exact (N <= 2^24 is required) ; loss = sum(row_loss) / count ; acc = hits / count
 *   count == 0  : loss = acc = count = 0 and every gradient is 0.  THIS DEVIATES FROM TORCH, which returns NaN for a batch
 *                 without a counted target; a NaN here would poison the captured step's optimiser state.
 *   backward    : g_logits[n,v] = g_loss / max(count, 1) * (softmax - onehot).  `count` is the DEVICE scalar the forward wrote;
 *                 the host never sees it, so the pair can sit in a captured graph.
 * Deterministic (no atomics, fixed summation order).  With no row ignored every output has the bits of the entry point above:
 * count == N and g_loss / count is the same f32 division as g_loss / (float)N.
 * loss, acc and count of the forwards may each be NULL; count of the backwards may not.
 */
int kvq_ce_forward_ignore(const void* logits, const int64_t* target, int64_t N, int V, int64_t ld, int io_dtype, int64_t ignore_index,
                          float* row_loss, float* row_lse, int64_t* pred, float* loss, float* acc, float* count, void* stream);
int kvq_ce_forward_stats_ignore(const void* logits, const int64_t* target, int64_t N, int64_t ld, int io_dtype, const float* stats,
                                int tiles, int64_t ignore_index, float* row_loss, float* row_lse, int64_t* pred, float* loss,
                                float* acc, float* count, void* stream);
int kvq_ce_backward_ignore(const void* logits, const int64_t* target, const float* row_lse, const float* g_loss, const float* count,
                           int64_t ignore_index, int64_t N, int V, int64_t ld, int io_dtype, void* g_logits, void* stream);
/* An ignored row adds exactly 0 to bias_part. */
int kvq_ce_backward_bias_ignore(const void* logits, const int64_t* target, const float* row_lse, const float* g_loss,
                                const float* count, int64_t ignore_index, int64_t N, int V, int64_t ld, int io_dtype, void* g_logits,
                                float* bias_part, size_t part_bytes, void* stream);
/* per_sentence[b] = hits over sentence b's counted tokens / their number; 0 for a sentence without a counted token. */
int kvq_seq_acc_ignore(const int64_t* pred, const int64_t* target, int64_t B, int S, int64_t ignore_index, float* per_sentence,
                       void* stream);

/* ------------------------------------------------------------------------------------------------
 * Memory-bound pieces of the BERT blocks (HuggingFace modeling_bert.py as used by models/bagon/Bagon.py:24-31),
 * one kernel pass per block boundary; bf16 or f32 activations, f32 arithmetic.  `seed`/`site` key the counter-based
 * dropout generator (Philox4x32-10): forward and backward regenerate the same mask, nothing is stored.
 */

/* BertSelfOutput / BertOutput (:282-293, :340-352):  out = LayerNorm(dropout(y) + resid).
 *   y, resid (may be NULL), out, pre [N,H] io dtype; gamma, beta [H] f32; pre (may be NULL) = dropout(y)+resid as stored;
 *   mean, rstd [N] f32 (may be NULL).  H %% 4 == 0, H <= 4096 (backward: H <= 3072). */
int kvq_dropout_residual_ln_fwd(const void* y, const void* resid, const float* gamma, const float* beta, int64_t N, int H,
                                float eps, float p_drop, uint64_t seed, uint32_t site, int io_dtype, void* out, void* pre,
                                float* mean, float* rstd, void* stream);
size_t kvq_ln_bwd_workspace_bytes(int64_t N, int H);
/* g_y = d/dy, g_resid = d/dresid (either may be NULL); g_gamma, g_beta [H] in param_grad_dtype, overwritten or
 * accumulated into (accumulate != 0); either may be NULL.  g_bias_prev [H] (may be NULL) receives the column sums of g_y,
 * i.e. the bias gradient of the dense layer that produced y (BertSelfOutput.dense / BertOutput.dense). */
int kvq_dropout_residual_ln_bwd(const void* g_out, const void* pre, const float* mean, const float* rstd, const float* gamma,
                                int64_t N, int H, float p_drop, uint64_t seed, uint32_t site, int io_dtype, void* g_y,
                                void* g_resid, void* g_gamma, void* g_beta, void* g_bias_prev, int param_grad_dtype, int accumulate,
                                void* ws, size_t ws_bytes, void* stream);

/* out[c] (= or +=) scale * sum_n x[n,c]   (bias gradients).  x [N, ld] in_dtype, out [C] out_dtype. */
size_t kvq_colsum_workspace_bytes(int64_t N, int64_t C);
int kvq_colsum(const void* x, int64_t N, int64_t C, int64_t ld, int in_dtype, void* out, int out_dtype, float scale,
               int accumulate, void* ws, size_t ws_bytes, void* stream);

/* Batched reductions (one launch for many small sums): item i computes
 *   dst[c] = scale * sum_{p < count} src[p*ld + c] (+ dst[c] when accumulate != 0),  c < cols.
 * The backward of one BERT layer yields 8-14 of these (split-K slabs of the weight-gradient GEMMs, per-workgroup partials of
 * the LayerNorm gamma/beta and bias gradients: kvq_*_partial below); run one by one each is a launch-latency-bound kernel.
 * Rows are summed in index order, so results are deterministic.  Long rows with count <= 32 (split-K slabs) take a
 * vectorised path when cols, ld %% 8 == 0 and src/dst are 16-byte aligned. */
#define KVQ_REDUCE_MAX_ITEMS 32
typedef struct kvq_reduce_item {
    const void* src;
    void* dst;
    int64_t count, cols, ld;
    float scale;
    int32_t src_dtype, dst_dtype, accumulate;
} kvq_reduce_item;
int kvq_reduce_batch(const kvq_reduce_item* items, int n, void* stream);

/* First halves of kvq_dropout_residual_ln_bwd / kvq_colsum: everything except the final sums over the partial rows, which the
 * caller hands to kvq_reduce_batch.  LayerNorm partials: part [kvq_ln_bwd_partial_rows(N)][3H] f32 = [dbias_prev | dgamma | dbeta]
 * (the dbias_prev third only when want_dbias); column-sum partials: part [kvq_colsum_partial_rows(N)][C] f32.
 * part_bytes >= kvq_ln_bwd_workspace_bytes(N,H) / kvq_colsum_workspace_bytes(N,C). */
int64_t kvq_ln_bwd_partial_rows(int64_t N);
int kvq_dropout_residual_ln_bwd_partial(const void* g_out, const void* pre, const float* mean, const float* rstd,
                                        const float* gamma, int64_t N, int H, float p_drop, uint64_t seed, uint32_t site,
                                        int io_dtype, void* g_y, void* g_resid, int want_dbias, void* part, size_t part_bytes,
                                        void* stream);
/* BertEmbeddings (modeling_bert.py:53-110) forward in one pass and the LayerNorm half of its backward:
 *   out = dropout(LayerNorm(word[ids[n]] + (pos[n %% S] + type_row)))   -- note: dropout AFTER the LayerNorm here
 *   ids [N] int64 (an id outside [0, V) is clamped; torch raises), word [V,H], pos [>= S, H], type_row [H] in the io dtype;
 *   pre [N,H] = the LayerNorm input as stored (backward re-reads it), mean / rstd [N] f32.
 * kvq_ln_dropout_bwd_partial: g_y = d/d(LayerNorm input) for that block (the mask of (seed, site) applies to the incoming
 * gradient g_out); part as in kvq_dropout_residual_ln_bwd_partial with the dbias third unused. */
int kvq_embed_ln_fwd(const int64_t* ids, const void* word, const void* pos, const void* type_row, const float* gamma,
                     const float* beta, int64_t N, int S, int H, int64_t V, float eps, float p_drop, uint64_t seed, uint32_t site,
                     int io_dtype, void* out, void* pre, float* mean, float* rstd, void* stream);
int kvq_ln_dropout_bwd_partial(const void* g_out, const void* pre, const float* mean, const float* rstd, const float* gamma,
                               int64_t N, int H, float p_drop, uint64_t seed, uint32_t site, int io_dtype, void* g_y,
                               void* part, size_t part_bytes, void* stream);
int64_t kvq_colsum_partial_rows(int64_t N);
int kvq_colsum_partial(const void* x, int64_t N, int64_t C, int64_t ld, int in_dtype, void* part, size_t part_bytes, void* stream);

/* out[i] = sum_s part[s*n + i], f32 accumulate: combines the S split-K slabs of a weight-gradient GEMM.  n %% 4 == 0. */
int kvq_sum_slabs(const void* part, int S, int64_t n, int io_dtype, void* out, void* stream);

/* BertIntermediate activation (:325-337), erf GELU.  n elements, n %% 4 == 0. */
int kvq_gelu_fwd(const void* h, void* a, int64_t n, int io_dtype, void* stream);
int kvq_gelu_bwd(const void* h, const void* g_a, void* g_h, int64_t n, int io_dtype, void* stream);
/* kvq_gelu_bwd on a row-major [N, C] activation that also leaves bias_part [kvq_gelu_bwd_partial_rows(N)][C] f32 = partial
 * column sums of g_h (as stored, i.e. after rounding to the io dtype): the bias gradient of the dense layer in front of
 * the GELU (BertIntermediate, modeling_bert.py:298-310), finished by kvq_reduce_batch.  C %% 8 == 0, 16-byte aligned buffers. */
int64_t kvq_gelu_bwd_partial_rows(int64_t N);
int kvq_gelu_bwd_bias(const void* h, const void* g_a, void* g_h, int64_t N, int64_t C, int io_dtype, float* bias_part,
                      size_t part_bytes, void* stream);

/* BertSelfAttention / BertCrossAttention core (:111-204) for S_q, S_k <= 32 (bf16 with 16-byte aligned rows: <= 128, in 32-token
 * blocks) and head dim 64: softmax(q k^T * scale + mask) v with dropout on the probabilities.  q [B*Sq, ldq], k/v [B*Sk, ldk/ldv], out [B*Sq, ldo]; head h lives at columns h*64..;
 * mask [B,Sk] int64 (1 = attend) or NULL; causal != 0 adds key <= query.  lse [B,nh,Sq] (may be NULL).
 * A query row without any attended key (a mask row of zeros; under causal, a sentence whose first attended key lies behind the
 * query) has all-zero probabilities: its output row is exactly 0, its lse is log(1e-37), and in the backward it contributes
 * exactly 0 to g_q, g_k, g_v and the bias partials -- never NaN.  (HuggingFace's additive finfo.min mask gives uniform attention
 * over the padding there: a caller that needs that behaviour must not pass an all-zero mask row.) */
int kvq_attn_fwd(const void* q, const void* k, const void* v, const int64_t* mask, int B, int nh, int Sq, int Sk, int dh,
                 int ldq, int ldk, int ldv, int ldo, int causal, float scale, float p_drop, uint64_t seed, uint32_t site,
                 int io_dtype, void* out, float* lse, void* stream);
int kvq_attn_bwd(const void* q, const void* k, const void* v, const int64_t* mask, const void* g_out, int B, int nh, int Sq,
                 int Sk, int dh, int ldq, int ldk, int ldv, int ldo, int causal, float scale, float p_drop, uint64_t seed,
                 uint32_t site, int io_dtype, void* g_q, void* g_k, void* g_v, float* bias_part_q, float* bias_part_k,
                 float* bias_part_v, int ldp_q, int ldp_kv, void* stream);
/* The same backward with the forward's output `out` [B*Sq, ldo] and `lse` [B,nh,Sq] handed back: REQUIRED above 32 tokens (the
 * blocked kernels recompute the probabilities from lse and take delta = rowsum(g_out * out) from `out`; no atomics: one kernel
 * for g_q over (sentence, head, query block), one for g_k / g_v over (sentence, head, key block)); at <= 32 tokens both are
 * ignored and the call is kvq_attn_bwd. */
int kvq_attn_bwd_saved(const void* q, const void* k, const void* v, const int64_t* mask, const void* out, const float* lse,
                       const void* g_out, int B, int nh, int Sq, int Sk, int dh, int ldq, int ldk, int ldv, int ldo, int causal,
                       float scale, float p_drop, uint64_t seed, uint32_t site, int io_dtype, void* g_q, void* g_k, void* g_v,
                       float* bias_part_q, float* bias_part_k, float* bias_part_v, int ldp_q, int ldp_kv, void* stream);
/* bias_part_* (each may be NULL): per-batch column sums of g_q / g_k / g_v, [B][ldp_q] resp. [B][ldp_kv] f32, columns
 * 0 .. nh*64 -- the partial rows of the q/k/v projection bias gradients (modeling_bert.py:83-85 biases), to be finished by
 * kvq_reduce_batch over the B rows.  The MFMA kernels emit them on the way out; the other flavours run a column-sum pass. */

/* The attention PROBABILITIES of the same operands (one layer's `attentions` / `cross_attentions` of HuggingFace's
 * output_attentions=True, modeling_bert.py:139-204), without dropout -- an evaluation quantity: launches of their own, the forward
 * kernels are untouched.  q / k / mask / causal / scale / io_dtype as in kvq_attn_fwd; v is part of the operand description and is
 * not read.  Either or both of
 *   probs [B, nh, Sq, Sk] f32   the per-sentence probabilities: the UNROUNDED f32 softmax of the f32 score accumulation (what the
 *                               forward kernels hold before they round P to bf16 for P.V);
 *   table [nh, Sq, Sk]   f64    table += sum over the B sentences of this call (the mean over everything seen is table / count,
 *                               taken by the caller at the end).
 * A query row without any attended key has all-zero probabilities, as in kvq_attn_fwd, and still counts as a sentence.
 * Deterministic, no floating-point atomics: a workgroup owns a contiguous run of sentences of one head, sums them in ascending
 * order in f64 registers and leaves one slab in `ws`; a second kernel adds the slabs in ascending order into `table`.  Two calls on
 * the same inputs give the same bits.  ws: kvq_attn_probs_workspace_bytes(B, nh, Sq, Sk) bytes, 16-byte aligned, needed only with a
 * table.  Kernels only (no memset / memcpy nodes): capturable.
 * Flavours: bf16 with 16-byte aligned rows and Sq, Sk <= 32: scores on v_mfma_f32_32x32x16_bf16; f32 (and unaligned bf16) <= 32: the
 * LDS-tile kernel; bf16 with 33..128 tokens on either side: REQUIRES lse [B, nh, Sq] of kvq_attn_fwd on the same operands
 * (P = exp(s - lse) per 32-key block, then each row is normalised by its own sum, which removes lse's rounding); at <= 32
 * tokens lse is ignored and may be NULL.  Whatever kvq_attn_fwd refuses is refused here with the same status. */
size_t kvq_attn_probs_workspace_bytes(int B, int nh, int Sq, int Sk);
int kvq_attn_probs(const void* q, const void* k, const void* v, const int64_t* mask, const float* lse, int B, int nh, int Sq, int Sk,
                   int dh, int ldq, int ldk, int ldv, int causal, float scale, int io_dtype, float* probs, double* table, void* ws,
                   size_t ws_bytes, void* stream);

/* bf16 attention flavour: 2 (default) = MFMA kernels (v_mfma_f32_32x32x16_bf16 for all five products), 1 = packed-dot
 * kernels (v_dot2c_f32_bf16); both round probabilities / dS to bf16 before P.V, dS.K, dS^T.Q, P^T.dO.  0 = convert-and-fma
 * kernels (f32 probabilities).  All flavours draw the same dropout mask.  f32 io always uses the f32 kernels.  The selection is
 * per calling thread (a test / checker facility: the product path never changes it). */
int kvq_attn_set_variant(int variant);

/* ---- bf16 MFMA GEMM family, all three operand layouts of one nn.Linear's forward / backward (csrc/kvq_gemm2.hip) ----------
 * Replaces, for y = x . W^T + b of every BertSelfAttention / BertSelfOutput / BertIntermediate / BertOutput / LM-head linear
 * reached from models/bagon/Bagon.py:46-53 and models/shelgon3/Shelgon.py:52,71 (modeling_bert.py:139-352,483-497):
 *   KVQ_GEMM_NT  C[M,N] = A[M,K] . B[N,K]^T     forward        (x, W)         torch: F.linear
 *   KVQ_GEMM_NN  C[M,N] = A[M,K] . B[K,N]       input gradient (gy, W)        autograd: grad_output.mm(weight)
 *   KVQ_GEMM_TN  C[M,N] = A[K,M]^T . B[K,N]     weight gradient (gy, x)       autograd: grad_output.t().mm(input)
 * bf16 operands and result, f32 accumulation (v_mfma_f32_16x16x32_bf16), optional bias[N] (bf16) and C += (accumulate != 0).
 * K %% 64 == 0; M, N, lda, ldb, ldc %% 8 == 0; 16-byte aligned operands; row-major with the given leading dimensions.
 * `tile` picks the workgroup tile: the caller chooses it so that the tile count fills the 256 CUs (kvq.nnops.pick_tile is the caller's rule).
 * A grouped launch runs up to 16 problems of ONE layout as a single grid (e.g. the weight gradients of two BERT layers:
 * ~250 tiles of 256 x 256, one per CU over the whole token contraction -- no split-K, no partial slabs). */
#define KVQ_GEMM_NT 0
#define KVQ_GEMM_NN 1
#define KVQ_GEMM_TN 2
#define KVQ_GEMM_TILE_128x192 0   /* 8 waves; 256 tiles for [8192, 768] outputs */
#define KVQ_GEMM_TILE_128x256 1   /* 8 waves */
#define KVQ_GEMM_TILE_256x192 2   /* 8 waves */
#define KVQ_GEMM_TILE_256x256 3   /* 8 waves */
#define KVQ_GEMM_TILE_64x128 4    /* 4 waves, two workgroups per CU: outputs too small to give every CU a larger tile (the reference's own
                                   * batches: 12 tokens x 64..128 sentences, models/shelgon3/Trainer.py:82) */
#define KVQ_GEMM_TILE_128x192H 5  /* 4 waves, two ring slots, 80 KiB: TWO workgroups per CU (one wave per SIMD each) whose start-up and
                                   * epilogue run under the other's k loop.  Round-5 experiment: ahead on hot operands, behind inside the
                                   * training step (profiles/r05_gemm_ceiling.md); no caller picks it by itself */
/* OR-ed into `tile` (layout NT, one problem, no accumulate, M and N at least one tile, K >= 192): the PERSISTENT form -- one
 * workgroup per CU walks its tiles, the k-tiles of successive tiles form one uninterrupted LDS-DMA stream and the epilogue
 * goes from the accumulator registers straight to memory; pays when a CU owns two or more tiles. */
#define KVQ_GEMM_PERSISTENT 0x100
typedef struct kvq_gemm_problem {
    const void* A;
    const void* B;
    void* C;
    const void* bias;     /* bf16 [N] or NULL */
    int M, N, K;
    int lda, ldb, ldc;
    int accumulate;
} kvq_gemm_problem;
int kvq_gemm_bf16(const void* A, const void* B, const void* bias, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                  int layout, int tile, int accumulate, void* stream);
/* The any-shape member of the family (csrc/kvq_gemm_any.hip): same layouts and meaning, NO divisibility or 16-byte alignment
 * requirement (any M, N, K, leading dimensions; 2-byte aligned operands); f32 accumulation in ascending k on the vector unit.
 * For the launch-latency-sized products that do not meet kvq_gemm_bf16's requirements (token counts that are not multiples of
 * 64, 9-code Gumbel logits, ...), so that no product of the bf16 step leaves the library. */
int kvq_gemm_any_bf16(const void* A, const void* B, const void* bias, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                      int layout, int accumulate, void* stream);
int kvq_gemm_grouped_bf16(const kvq_gemm_problem* problems, int n_problems, int layout, int tile, void* stream);
/* A grouped launch (layout KVQ_GEMM_TN only) whose problems carry their own tile: tiles[i] is KVQ_GEMM_TILE_256x256 or _128x256.
 * One grid; the 256 x 256 tiles are numbered -- and so dispatched -- first.  Every output element is what kvq_gemm_grouped_bf16
 * stores for the same problem and tile, bit for bit.  For an output of more than one but less than two rounds of 256 x 256
 * tiles (the LM-head weight gradient): a row slice that fills the CUs once with 256 x 256 tiles, the remaining rows as
 * 128 x 256 tiles in a second, shorter round.  Same limits as kvq_gemm_grouped_bf16 (16 problems). */
int kvq_gemm_grouped_mixed_bf16(const kvq_gemm_problem* problems, const int* tiles, int n_problems, int layout, void* stream);
/* BertIntermediate in one kernel (modeling_bert.py:325-337), layout NT: Hout = A.B^T + bias (kept for backward) and
 * Aout = gelu(Hout as rounded to bf16) -- exact-erf GELU (erf to 1.2e-7).  tile: KVQ_GEMM_TILE_256x192 or _128x256 (optionally
 * | KVQ_GEMM_PERSISTENT). */
/* The dense layer in front of a residual LayerNorm (BertSelfOutput / BertOutput, modeling_bert.py:282-296, 339-352), layout NT:
 * C = dropout(A.B^T + bias, p_drop) + R, rounded as kvq_dropout_residual_ln_fwd rounds its `pre` (the dense output to bf16, times the
 * keep scale, plus the residual, to bf16) and with ITS masks (seed + the kvq_set_seed_offset word, `site`, element index): C is
 * bit for bit the `pre` that kernel would store, so LayerNorm forward becomes kvq_dropout_residual_ln_fwd(C, NULL, p = 0) -- half the
 * bytes -- and backward is unchanged.  R: [M, N] bf16, row stride ldc.  tile: KVQ_GEMM_TILE_128x192, _128x256 or _64x128. */
int kvq_gemm_bf16_dropres(const void* A, const void* B, const void* bias, const void* R, void* C, int M, int N, int K, int lda, int ldb,
                          int ldc, int tile, float p_drop, uint64_t seed, uint32_t site, void* stream);
int kvq_gemm_bf16_gelu(const void* A, const void* B, const void* bias, void* Hout, void* Aout, int M, int N, int K, int lda, int ldb,
                       int ldc, int tile, void* stream);
/* Its backward through the activation, layout NN: C = (A.B) * gelu'(H)  (A = gradient of BertOutput.dense's output, B = its
 * weight [K,N], H = the saved pre-activation [M,N], row stride ldc) plus part[t][n] = sum over the rows of row-tile t of the
 * bf16 values stored in C: the partial rows of BertIntermediate's bias gradient (finish with kvq_reduce_batch over
 * kvq_gemm_dgelu_partial_rows(M, tile) rows).  Replaces the dgrad GEMM + the elementwise gelu-backward + bias column sums. */
int64_t kvq_gemm_dgelu_partial_rows(int64_t M, int tile);
int kvq_gemm_bf16_dgelu(const void* A, const void* B, const void* H, void* C, float* part, size_t part_bytes, int M, int N, int K,
                        int lda, int ldb, int ldc, int tile, void* stream);

/* LM head with the forward half of the reconstruction loss in the GEMM epilogue (models/shelgon3/Trainer.py:94-101 after
 * BertLMPredictionHead.decoder, modeling_bert.py:483-497):  C[M, ldc] (bf16) = A[M,K] . B[N,K]^T + bias  (layout NT, 256 x 256
 * tiles) and stats [M][ceil(N/256)][4] f32 = per row and tile (max, sum exp(x - max), first arg-max, -) of the values as stored,
 * over the columns < V (vocabulary padding excluded).  kvq_ce_forward_stats turns them into loss / lse / arg-max / accuracy. */
size_t kvq_gemm_ce_stats_bytes(int M, int N);
int kvq_gemm_bf16_ce(const void* A, const void* B, const void* bias, void* C, int M, int N, int K, int lda, int ldb, int ldc, int V,
                     float* stats, size_t stats_bytes, void* stream);

/* ---- fp8 (OCP e4m3fn) forward GEMMs: extension named by BASELINE.json configs[4]; the reference is f32 throughout -> off by default.
 *   y = x . W^T + b of a BERT linear (modeling_bert.py:139-352) as  (sat(x sx) . sat(W sw)^T) / (sx sw) + b,  s = 448 / amax|.|
 *   per tensor, computed in the same step from the tensor that is quantised (no amax history).  Backward stays bf16 (but see the
 *   input-gradient option below: kvq_gemm_fp8_nt_ex).
 * kvq_fp8_quantize: one bf16 matrix [rows, cols] (row stride ld) -> dense fp8 [rows, cols]; amax, scale: device scalars (written).
 * kvq_fp8_quantize_segments: ranges [seg_off[s], +seg_n[s]) (elements; device arrays; multiples of 16) of one bf16 buffer ->
 *   the same ranges of an fp8 buffer, one amax / scale per range: all GEMM weights of the model in two launches.
 * kvq_gemm_fp8_nt: C[M,N] bf16 = (A8[M,K] . B8[N,K]^T) / (scale_a[0] scale_b[0]) + bias;  K %% 128 == 0, lda, ldb %% 16 == 0
 *   (fp8 elements), on v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales (2x the bf16 matrix rate). */
int kvq_fp8_quantize(const void* x_bf16, int64_t rows, int cols, int64_t ld, void* out_fp8, float* amax, float* scale, void* stream);
/* Activations, one pass ("delayed scaling"): per call site a device record of kvq_fp8_state_floats() floats, [0] = scale
 * (initialise to 1), the rest per-workgroup amax partials (initialise to 0): quantise with the site's scale and leave this
 * tensor's amax in the partials; kvq_fp8_update_scales (once per step, nsites consecutive records) sets
 * scale = 448 / (amax * headroom) and clears the partials (headroom 0: clears only -- after a forward whose amax must not
 * count, e.g. an evaluation batch).  Values beyond the previous step's range saturate at +-448. */
int kvq_fp8_state_floats(void);
int kvq_fp8_quantize_delayed(const void* x_bf16, int64_t rows, int cols, int64_t ld, void* out_fp8, float* state, void* stream);
int kvq_fp8_update_scales(float* state, int nsites, float headroom, void* stream);
int kvq_fp8_quantize_segments(const void* src_bf16, const int64_t* seg_off, const int64_t* seg_n, int nseg, int64_t max_seg_n,
                              void* dst_fp8, float* amax, float* scale, void* stream);
/* The same inside a training step: the per-segment amax (and with it the scale) is refreshed only when the DEVICE-resident step
 * count *step_count_u64 is a multiple of `period`; on the steps between, the segments are quantised with the scale they have
 * (values that outgrew it saturate at +-448).  Weights move by ~lr per step: a period of 16 saves one of the two passes over the
 * weights on 15 steps of 16. */
/* (period < -1: ALSO the conversion pass runs only on steps that are multiples of -period -- for a caller whose optimiser kernel
 * writes the fp8 bytes itself on the other steps: kvq_adam_step_dev_fp8.) */
int kvq_fp8_quantize_segments_periodic(const void* src_bf16, const int64_t* seg_off, const int64_t* seg_n, int nseg, int64_t max_seg_n,
                                       void* dst_fp8, float* amax, float* scale, const void* step_count_u64, int period, void* stream);
int kvq_gemm_fp8_nt(const void* A8, const void* B8, const float* scale_a, const float* scale_b, const void* bias, void* C, int M, int N,
                    int K, int lda, int ldb, int ldc, void* stream);
/* Round 5 -- the fp8 copy of an activation written by the kernel that PRODUCES it, so that the fp8 GEMM reading it next needs no
 * quantisation pass: each of these writes, beside its bf16 result, exactly the bytes kvq_fp8_quantize_delayed(result, state) would
 * write (the site's scale of the previous step) and notes the result's amax in the state's partial slots (atomic maxima: any
 * number of workgroups).  The caller runs kvq_fp8_update_scales once per step as before.
 *   kvq_dropout_residual_ln_fwd_fp8 : LayerNorm output -> the QKV / cross-attention query / BertIntermediate projections
 *   kvq_attn_fwd_fp8                : attention context (at most 32 tokens, the MFMA kernel: kvq_attn_fwd_fp8_ok) -> BertSelfOutput.dense
 *   kvq_gemm_fp8_nt_gelu            : BertIntermediate on the fp8 matrix cores with the GELU epilogue of kvq_gemm_bf16_gelu, and
 *                                     (Aout_fp8 != NULL) the fp8 copy of gelu(h) -> BertOutput.dense */
int kvq_dropout_residual_ln_fwd_fp8(const void* y, const void* resid, const float* gamma, const float* beta, int64_t N, int H,
                                    float eps, float p_drop, uint64_t seed, uint32_t site, void* out, void* pre, float* mean, float* rstd,
                                    void* out_fp8, float* fp8_state, void* stream);
int kvq_attn_fwd_fp8_ok(int Sq, int Sk);
int kvq_attn_fwd_fp8(const void* q, const void* k, const void* v, const int64_t* mask, int B, int nh, int Sq, int Sk, int dh,
                     int ldq, int ldk, int ldv, int ldo, int causal, float scale, float p_drop, uint64_t seed, uint32_t site,
                     void* out, float* lse, void* out_fp8, int ld8, float* fp8_state, void* stream);
int kvq_gemm_fp8_nt_gelu(const void* A8, const void* B8, const float* scale_a, const float* scale_b, const void* bias, void* Hout, void* Aout,
                         void* Aout_fp8, int ld8, float* fp8_state, int M, int N, int K, int lda, int ldb, int ldc, void* stream);

/* ---- fp8 input-gradient GEMMs (option, off by default): gx[N,K] = gy[N,M] . W[M,K] as the NT product of gy in OCP e5m2 (the
 * range gradients need) and the byte-transposed e4m3 weight mirror W^T[K,M] -- same scale, no requantisation.
 * Operand formats of the fp8 GEMM / the quantisation passes: */
#define KVQ_FP8_E4M3 0       /* OCP e4m3fn, largest value 448 */
#define KVQ_FP8_E5M2 1       /* OCP e5m2, largest value 57344 */
/* kvq_gemm_fp8_nt_ex: C[M,N] bf16 (+)= (A8[M,K] . B8[N,K]^T) / (scale_a[0] scale_b[0]) + bias.  a_format: the format of A8
 *   (KVQ_FP8_E4M3 | KVQ_FP8_E5M2); B8 is e4m3.  accumulate != 0: the product (+ bias), rounded to bf16, is added to the C that is
 *   there, in f32, and rounded once more (the epilogue of kvq_gemm_bf16's accumulate).  Refusals as kvq_gemm_fp8_nt: K %% 128,
 *   lda / ldb %% 16 (fp8 elements), M, N, ldc %% 8, 16-byte aligned operands.  a_format = KVQ_FP8_E4M3, accumulate = 0 launches the
 *   kernel of kvq_gemm_fp8_nt (same bits). */
int kvq_gemm_fp8_nt_ex(const void* A8, const void* B8, const float* scale_a, const float* scale_b, const void* bias, void* C,
                       int M, int N, int K, int lda, int ldb, int ldc, int a_format, int accumulate, void* stream);
/* The tile kvq_gemm_fp8_nt / kvq_gemm_fp8_nt_ex launch for an [M, N] output on the current device: KVQ_GEMM_TILE_128x256, or
 *   KVQ_GEMM_TILE_128x192 where that fills more CUs (the same function decides for the launch).  -1 for M or N <= 0.  No launch. */
int kvq_gemm_fp8_tile(int M, int N);
/* The quantisation calls above with the target format as an argument (fmt = KVQ_FP8_E4M3: the bytes of the calls above);
 * round to nearest even, saturating at the format's largest value, a NaN stays a NaN.  Rows may be strided (ld >= cols, cols and
 * ld %% 8 == 0); rows of a multiple of 16 columns are written in 16-byte pieces.  Kernel launches only: all three can be captured.
 *   kvq_fp8_quantize_fmt         : amax pass + quantise pass, scale = max(fmt) / amax of the tensor itself (amax, scale: written).
 *                                  An inf in the tensor does NOT saturate here (nor in kvq_fp8_quantize): amax = inf, scale = 0,
 *                                  every finite value becomes a signed zero and the inf itself 0 * inf = NaN
 *   kvq_fp8_quantize_delayed_fmt : one pass with the record's scale, this tensor's amax left in the record's partials (the record
 *                                  layout of kvq_fp8_quantize_delayed).  out_fp8 == NULL: only the amax is noted (calibration)
 *   kvq_fp8_update_scales_fmt    : scale = max(fmt) / (amax * headroom) for nsites consecutive records of ONE format; a record
 *                                  whose partials are all 0 keeps its scale; headroom 0 only clears */
int kvq_fp8_quantize_fmt(const void* x_bf16, int64_t rows, int cols, int64_t ld, void* out_fp8, float* amax, float* scale, int fmt,
                         void* stream);
int kvq_fp8_quantize_delayed_fmt(const void* x_bf16, int64_t rows, int cols, int64_t ld, void* out_fp8, float* state, int fmt,
                                 void* stream);
int kvq_fp8_update_scales_fmt(float* state, int nsites, float headroom, int fmt, void* stream);
/* Byte transpose of an fp8 matrix: dst8[c, r] = src8[r, c], src8 [rows, cols] with row stride ld_src, dst8 [cols, rows] with row
 * stride ld_dst (bytes); rows, cols, ld_src, ld_dst multiples of 16, 16-byte aligned buffers that do not overlap.
 * kvq_fp8_transpose_segments: nseg dense matrices in one launch -- segment s is [seg_rows[s], seg_cols[s]] at src8 + src_off[s]
 *   and goes, transposed and dense, to dst8 + dst_off[s] (device arrays of int64).  EVERY table entry must be a multiple
 *   of 16: the tables live on the device, the host cannot check them, and the result for any other entry is undefined (the
 *   kernel stays inside the segments, but its 16-byte accesses are misaligned and the dense layout is wrong); max_tiles >= ceil(rows / 128) * ceil(cols / 128) of every
 *   segment.  One launch for every weight of a model. */
int kvq_fp8_transpose(const void* src8, int rows, int cols, int64_t ld_src, void* dst8, int64_t ld_dst, void* stream);
int kvq_fp8_transpose_segments(const void* src8, void* dst8, const int64_t* src_off, const int64_t* seg_rows, const int64_t* seg_cols,
                               const int64_t* dst_off, int nseg, int64_t max_tiles, void* stream);

/* torch.optim.Adam step (models/shelgon3/main.py:91: lr, weight_decay (L2, coupled), amsgrad) on flat buffers.
 *   p, m, v [, vmax] f32; g grad_dtype (scaled by grad_scale first); shadow_bf16 (may be NULL) receives bf16(p_new).
 *   step >= 1 is the 1-based step count for bias correction (1 - beta1^step and sqrt(1 - beta2^step) are formed in double and
 *   rounded to f32 once, as kvq_step_state_advance forms them).  Any n >= 1 (16-byte aligned buffers; the last n %% 4 elements take a
 *   scalar path: the 9-code Gumbel bias of the reference's analysis run). */
/* kvq_adam_step_dev that also writes the fp8 (e4m3) mirror of the GEMM weights inside [first_element, first_element + n) of the flat
 * parameter buffer: w8_mirror is indexed like that buffer (one byte per element), span_segment[element >> 11] = the quantisation
 * segment covering that 2048-element span (-1 none, -2 several things: the kernel then walks seg_off / seg_n), seg_scale the segments'
 * current scales.  The bytes are kvq_fp8_quantize_segments' for the bf16 value the update stores in the shadow. */
int kvq_adam_step_dev_fp8(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                          const void* step_state, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                          void* w8_mirror, const int* span_segment, const float* seg_scale, const int64_t* seg_off, const int64_t* seg_n,
                          int nseg, int64_t first_element, void* stream);
int kvq_adam_step(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                  void* stream);


/* ---- device-resident step state (hipGraph-friendly training step) ------------------------------------------------------
 * step_state: 24 bytes of device memory, zero-initialised = "no optimiser step applied yet":
 *     struct { uint64_t step; float lr, bc1, bc2s, pad; }
 * (its optional companion, the 32-byte gradient guard state of a step that measures / clips its gradient norm: "gradient guard" below)
 * kvq_step_state_advance   one-thread kernel run at the start of an optimiser step: step += 1, lr = lr0 * gamma^(number of
 *                          milestones <= step-1)  (torch MultiStepLR ticked once per finished step, Trainer.py:114-115),
 *                          bc1 = 1 - beta1^step, bc2s = sqrt(1 - beta2^step).  At most 8 milestones (host array).
 * kvq_adam_step_dev        kvq_adam_step reading lr / bias corrections from the step state instead of taking them by value.
 * kvq_set_seed_offset      per calling thread: every dropout-bearing kernel that thread launches afterwards (kvq_dropout,
 *                          kvq_dropout_residual_ln_*, kvq_attn_*) uses seed + step_state->step, read on the device at run
 *                          time; NULL switches it off.  A step captured once in a hipGraph then replays with fresh masks,
 *                          the right learning rate and bias corrections, with nothing patched from the host.
 * kvq_dropout              out = x * keep/(1-p) for the Philox mask of (seed, site); element i draws from call i/4 like the
 *                          other kernels.  Forward and (applied to the gradient) backward of a plain dropout.  n %% 4 == 0. */
int kvq_step_state_advance(void* step_state, float lr0, float gamma, const int64_t* milestones, int n_milestones, float beta1,
                           float beta2, void* stream);
int kvq_adam_step_dev(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                      const void* step_state, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                      void* stream);
int kvq_set_seed_offset(const void* step_state);
int kvq_dropout(const void* x, int64_t n, float p_drop, uint64_t seed, uint32_t site, int io_dtype, void* out, void* stream);
/* Zero 1..4 byte ranges (16-byte aligned pointers and sizes) in one launch: the word / position / token-type gradient tables of
 * BertEmbeddings (modeling_bert.py:53-58) before kvq_embed_grad and the batched reductions add into them. */
int kvq_zero_ranges(void* const* ptrs, const int64_t* bytes, int n, void* stream);

/* ---- gradient guard: global gradient norm, clipping by it, and the skip of a non-finite step (csrc/kvq_gradnorm.hip) ---------
 * guard state: 32 bytes of device memory beside the step state, zero-initialised:
 *     struct { double sumsq; float norm, coef; uint32_t skip, pad; uint64_t skipped; }
 * Between backward and Adam a step runs, on its own stream and with no host round trip (so a captured step replays it unchanged):
 * kvq_grad_sumsq_partials  P = 2048, the number of f64 partial sums one kvq_grad_sumsq_partial call writes.  A constant of the
 *                          library, NOT derived from the device's CU count: the same buffer gives the same bits on every box.
 * kvq_grad_sumsq_partial   partials[0..P) = partial sums of g[i]^2 over n >= 1 elements (grad_dtype KVQ_F32 / KVQ_BF16, g 16-byte
 *                          aligned, n_partials must be P).  Deterministic: a fixed grid of P workgroups, elements [8c, 8c+8) go to
 *                          thread c mod (256 P) of that grid, the last n %% 8 elements take a scalar path in thread 0; no float
 *                          atomics.  The 8 squares of a 16-byte chunk are added in f32, everything above in f64.  One call per
 *                          piece of the gradient, each into its own P slots of one partials buffer.
 * kvq_grad_guard_finalize  one workgroup: sumsq = sum of the n_total partials (a multiple of P; thread t of 256 adds partials t,
 *                          t + 256, ... in index order, then a fixed tree, all f64), norm = (float)sqrt(sumsq).  sumsq finite:
 *                          coef = min(1, max_norm / (norm + 1e-6f)) (torch.nn.utils.clip_grad_norm_), skip = 0; max_norm = +inf
 *                          gives coef = 1: measure and guard only.  sumsq inf or NaN (a non-finite gradient, or the overflow of
 *                          an f32 square): coef = 0, skip = 1, skipped += 1.  sumsq, norm, coef and skip are written by every call.
 * kvq_adam_step_guarded[_fp8]  kvq_adam_step_dev[_fp8] plus the guard state, read on the device: the gradient is scaled by
 *                          grad_scale * guard->coef; with guard->skip set the kernel returns before its first store, so p, m, v,
 *                          vmax, the bf16 shadow and the fp8 mirror keep their bits and neither weight decay nor the moment decays
 *                          run.  (kvq_adam_step* pass no guard: their code path is unchanged.)
 * A skipped step still runs kvq_step_state_advance: dropout masks and the learning-rate schedule move on, and bc1 / bc2s of the
 * step state therefore count ATTEMPTED steps, not applied ones. */
int kvq_grad_sumsq_partials(void);
int kvq_grad_sumsq_partial(const void* g, int64_t n, int grad_dtype, double* partials, int n_partials, void* stream);
int kvq_grad_guard_finalize(const double* partials, int n_total, float max_norm, void* guard, void* stream);
int kvq_adam_step_guarded(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                          const void* step_state, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                          const void* guard, void* stream);
int kvq_adam_step_guarded_fp8(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                              const void* step_state, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                              void* w8_mirror, const int* span_segment, const float* seg_scale, const int64_t* seg_off,
                              const int64_t* seg_n, int nseg, int64_t first_element, const void* guard, void* stream);

/* ---- parameter groups, decoupled weight decay and a learning-rate schedule in the step (csrc/kvq_adam.hip) ------------------------
 * Extension, off by default (TrainEngine(param_groups=..., decoupled_weight_decay=..., lr_warmup_steps=..., lr_decay=...)).
 * kvq_adam_step_grouped[_guarded]  kvq_adam_step_dev [kvq_adam_step_guarded] with a learning-rate scale s_j and a weight decay wd_j
 *                          per parameter GROUP j, looked up inside the one launch.  block_group[(first_element + e) >> 4] names
 *                          the group (0 .. n_groups - 1) of element e of the launch: one byte per 16-element block of the FLAT buffer
 *                          the range [first_element, first_element + n) was cut from (first_element a multiple of 16; the engine
 *                          starts and pads every parameter at multiples of 16, so a block never straddles two parameters).  Only the
 *                          bytes of the launch's own blocks are read.  A byte is NOT validated: the kernel uses its low four bits (so
 *                          no table byte can index outside its 16 table slots) and slots >= n_groups hold scale 0, decay 0 -- a
 *                          corrupt table trains silently under a wrong or a zero rate; building it right is the caller's job
 *                          (kvq.engine.param_group_blocks).  block_group == NULL: one group for the whole launch, entry 0
 *                          of the two tables (the aux parameters, a range inside one group): the work of kvq_adam_step_dev.
 *                          group_lr_scale / group_wd: n_groups (1 .. 16) floats of device memory each; NULL = every scale 1 /
 *                          every decay `weight_decay`.  Per element of group j, with lr, bc1, bc2s from the step state and the
 *                          gradient scaled by grad_scale [* guard->coef] as in kvq_adam_step_dev:  lr_j = fl(lr * s_j);
 *                            decoupled = 0  the statements of kvq_adam_step_dev with wd_j for weight_decay and lr_j for lr;
 *                            decoupled = 1  torch.optim.AdamW: p0 = fl(p * fl(1 - fl(lr_j * wd_j))), the moments from the scaled
 *                                           gradient alone, p' = fl(p0 - u) with kvq_adam_step_dev's u.
 *                          s_j = 0 does not freeze a group: its moments still move (and, decoupled = 0, see its weight decay).
 *                          Every s_j = 1, every wd_j = weight_decay, decoupled = 0: the bits of kvq_adam_step_dev / _guarded.
 *                          With guard->skip set nothing is stored.  There is no grouped form of the fp8-mirror entries.
 * kvq_step_state_advance_sched  kvq_step_state_advance with a warm-up and a decay: for the 1-based step t being applied
 *                            lr(t) = lr0 * gamma^k * warm * dec      (k as in kvq_step_state_advance; in double, rounded to f32 once)
 *                            warm  = t / W while t < W (W = warmup_steps > 0), else 1
 *                            x     = clamp((t - W) / (T - W), 0, 1)   (T = total_steps > W, required when decay_kind != 0)
 *                            dec   = 1 (decay_kind 0), 1 - (1 - r) x (1, linear), r + (1 - r) (1 + cos(pi x)) / 2 (2, cosine),
 *                                    r = min_ratio in [0, 1]
 *                          Past T the rate STAYS at r * lr0 * gamma^k: it does not climb again as torch's CosineAnnealingLR does.
 *                          warmup_steps = 0 and decay_kind = 0: the bits of kvq_step_state_advance.  The 24-byte state is unchanged. */
int kvq_adam_step_grouped(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                          const void* step_state, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                          const uint8_t* block_group, int64_t first_element, const float* group_lr_scale, const float* group_wd,
                          int n_groups, int decoupled, void* stream);
int kvq_adam_step_grouped_guarded(float* p, const void* g, float* m, float* v, float* vmax, void* shadow_bf16, int64_t n, int grad_dtype,
                                  const void* step_state, float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                  const uint8_t* block_group, int64_t first_element, const float* group_lr_scale, const float* group_wd,
                                  int n_groups, int decoupled, const void* guard, void* stream);
int kvq_step_state_advance_sched(void* step_state, float lr0, float gamma, const int64_t* milestones, int n_milestones, float beta1,
                                 float beta2, int64_t warmup_steps, int decay_kind, int64_t total_steps, float min_ratio, void* stream);

/* ---- gradient accumulation over the micro-batches of one optimiser step (csrc/kvq_accum.hip) ----------------------------------
 * Extension, off by default (TrainEngine(grad_accum=A)): forward and backward run A times, Adam once, on the MEAN of the A
 * gradients -- (loss / A).backward() A times, then opt.step().  The flat gradient is bf16 and rewritten by every backward, so the sum
 * is kept in an f32 accumulator of the same length.
 * accumulation state: 16 bytes of device memory, 8-byte aligned, zero-initialised:
 *     struct { uint64_t tick; uint32_t micro, pad; }
 * tick counts finished micro-steps and is never reset; micro = tick mod A is the position inside the current cycle.  tick is the
 * FIRST word on purpose: kvq_set_seed_offset takes a pointer to a uint64, and an accumulating step points the dropout seeds at this
 * state instead of the step state -- the optimiser step count does not move between the micro-steps of one cycle, which would
 * otherwise all draw the same masks.
 * kvq_grad_accumulate   with micro read on the device, for every i < n (n >= 1; g KVQ_BF16 or KVQ_F32; g and acc 16-byte aligned):
 *                           s      = micro == 0 ? (float) g[i] : acc[i] + (float) g[i]
 *                           acc[i] = micro == A - 1 ? s * (float)(1.0 / A) : s
 *                       The first micro-step of a cycle STORES and does not read acc: a NaN left by a skipped cycle, or memory
 *                       never written, does not survive, and no memset is needed.  The last one leaves the mean, which
 *                       kvq_adam_step_* (grad_scale 1) and kvq_grad_sumsq_partial read as a KVQ_F32 gradient.  The add and the
 *                       multiply are two roundings, never an FMA.  Elementwise, no atomics: deterministic.  A = 1: acc = g.
 * kvq_accum_advance     one thread: tick += 1, micro = micro + 1 == A ? 0 : micro + 1.  Once per micro-step, behind its last
 *                       kvq_grad_accumulate (and behind Adam on the last micro-step of a cycle).
 * Both are plain kernel launches on `stream`: a captured step replays them unchanged.  A null pointer, n < 1, A < 1 or another
 * dtype is refused before any launch. */
int kvq_grad_accumulate(const void* g, int64_t n, int grad_dtype, float* acc, const void* accum_state, int A, void* stream);
int kvq_accum_advance(void* accum_state, int A, void* stream);

/* ---- exponential moving average of the trained weights (csrc/kvq_weight_ema.hip) ----------------------------------------------
 * Extension, off by default (TrainEngine(weight_ema=decay)): beside the f32 master copy of every parameter Adam owns, an f32
 * average of what the optimiser left there, updated behind Adam inside the step; evaluation and the best-val checkpoints run under
 * it (TrainEngine.weight_ema_applied()).
 * weight-EMA state: 16 bytes of device memory, 8-byte aligned, zero-initialised:
 *     struct { uint64_t updates; float last_decay; uint32_t pad; }
 * updates counts the updates applied (a skipped step applies none); last_decay is the d of the last applied one, 0 for the first.
 * kvq_weight_ema_update   with t = updates read on the device, for every i < n (n >= 1; p and ema 16-byte aligned, disjoint):
 *                             t == 0:  ema[i] = p[i]                                  (a STORE: ema is not read)
 *                             t >= 1:  d = min((double) decay, (1.0 + t) / (10.0 + t))
 *                                      ema[i] = (float)(d * (double) ema[i] + (1.0 - d) * (double) p[i])
 *                         The first update does not read ema: memory never written, or a NaN, does not survive, and no memset is
 *                         needed (the idiom of kvq_grad_accumulate's first micro-step).  Every f64 operation is rounded on its own,
 *                         never an FMA, and the sum is rounded once to f32.  Elementwise, no atomics: deterministic.
 * kvq_weight_ema_advance  one thread: last_decay = t == 0 ? 0 : (float) d, then updates = t + 1.  Once per optimiser step, behind
 *                         its last kvq_weight_ema_update.
 * guard (both; may be NULL): the step's gradient guard state.  With guard->skip set the kernel returns before its first store, as
 *                         kvq_adam_step_guarded* do: the weights did not move, neither does their average nor the state.
 * kvq_weight_ema_swap     p[i] <-> ema[i] for every i < n, exactly (a second call restores every bit), and, where shadow_bf16 is
 *                         not NULL (8-byte aligned), shadow_bf16[i] = bf16(the new p[i]) with the rounding of the Adam kernels'
 *                         shadow store (nearest even, a NaN stays a NaN).  p == ema or overlapping buffers are refused.
 * All three are plain kernel launches on `stream`: a captured step replays them unchanged.  A null pointer, n < 1, decay outside
 * (0, 1) or a misaligned pointer is refused before any launch. */
int kvq_weight_ema_update(const float* p, float* ema, int64_t n, float decay, const void* ema_state, const void* guard, void* stream);
int kvq_weight_ema_advance(void* ema_state, float decay, const void* guard, void* stream);
int kvq_weight_ema_swap(float* p, float* ema, void* shadow_bf16, int64_t n, void* stream);

/* ---- codebook revival: a dead code restarts from an encoder output of the current batch (csrc/kvq_vq_revive.hip) -------------
 * Extension, absent from the reference, off by default (VectorQuantizer(revive_after=T)).  State per quantiser, device memory:
 *     idle [G, K] int32, zero-initialised: consecutive TRAINING steps in which code k of codebook g won no token
 *     counter, 16 bytes, 8-byte aligned, zero-initialised:   struct { uint32_t last, pad; uint64_t total; }
 * A training step runs three entry points on its own stream with no host round trip (kernels only: no memset, no memcpy, every
 * one may be captured), with T = revive_after >= 1:
 * kvq_vq_usage_flags     used[g, k] = 1 if some token n has idx[g, n] == k, else 0 (idx [G, N] int64, 1 <= N < 2^32).  An index
 *                        outside [0, K) is ignored (the fused tail leaves -1 for an all-NaN row).  EVERY element of used[G, K] is
 *                        written by the one launch: a workgroup owns 64 codes of one codebook and scans that codebook's indices;
 *                        no clear, no atomics.
 *                        Data parallel: the caller all-reduces `used` with MAX -- usage is a property of the global batch.
 * kvq_vq_revive_select   idle' = used ? 0 : min(idle + 1, INT32_MAX), written back for every code.  A code is DEAD when idle' >= T;
 *                        work on any other code ends after reading idle.  For a dead code, with c = g K + k:
 *                            r = philox4x32(c0 = c, c1 = 0, c2 = 0x52455649, c3 = 0x5eed; key = seed)     (4 x 32 bits)
 *                        where seed += the device step count when kvq_set_seed_offset is active (as every dropout kernel does);
 *                        0x52455649 ("REVI") is a site no dropout site reaches, those are a small counter.
 *                            owner rank = r.y %% world,      donor token n = ((uint64) r.x * N) >> 32
 *                            rows[g, k, :] = (float) z[g, n, :] on the owner (exact: z is f32 or bf16), +0.0f on every other rank
 *                        z [G, N, D] io_dtype (the layout kvq_vq_forward takes), rows [G, K, D] f32, both 16-byte aligned; rows of
 *                        codes that are not dead are not written.  16-byte accesses where the row pitch of z allows them (D %% 4 == 0
 *                        in f32, D %% 8 == 0 in bf16), one element at a time otherwise.
 *                        Data parallel: the caller all-reduces `rows` with SUM -- one rank contributes the value and the others
 *                        zeros, so the sum is exact in any order (a -0.0 becomes +0.0).
 * kvq_vq_revive_apply    after the codebook's own update of the step (Adam or EMA), before anything derived from the codebook is
 *                        rebuilt.  counter.last = number of dead codes (idle >= T), counter.total += last: written by every call,
 *                        by one workgroup, before the rows move.  For every dead code: E[g, k, :] = rows[g, k, :]; the row of the
 *                        Adam moments m, v, vmax = 0; ema_n[g, k] = 1 and ema_m[g, k, :] = rows[g, k, :] (what the constructor
 *                        gives a fresh code); idle = 0.  m, v, vmax, ema_n, ema_m may each be NULL.  A code that is not dead is not
 *                        touched at all.  E [G, K, D] f32 and rows 16-byte aligned; 16-byte accesses when D %% 4 == 0 and every
 *                        optional pointer is 16-byte aligned.
 * Deterministic: no floating-point atomics (no atomics at all), one wave per code, the same inputs give the same bits; with the
 * same seed, idle and (reduced) used every rank takes the same decisions.  Two dead codes may draw the same token: the lower
 * index then wins the arg-min tie, the other goes idle again and is redrawn T steps later under another step seed.  Revival is
 * not a gradient step: the gradient guard's skip does not gate it (nor does it gate the EMA update).
 * Every bad argument is refused before any launch: a NULL required pointer, N, K, D or G < 1, N >= 2^32, G K >= 2^31,
 * revive_after < 1, world < 1, rank outside [0, world), an unknown dtype, a misaligned z, rows or E. */
int kvq_vq_usage_flags(const int64_t* idx, int64_t N, int K, int G, int32_t* used, void* stream);
int kvq_vq_revive_select(const void* z, const int32_t* used, int64_t N, int K, int D, int G, int io_dtype, int revive_after,
                         uint64_t seed, int rank, int world, int32_t* idle, float* rows, void* stream);
int kvq_vq_revive_apply(const float* rows, int K, int D, int G, int revive_after, int32_t* idle, float* E, float* m, float* v,
                        float* vmax, float* ema_n, float* ema_m, void* counter, void* stream);


/* ---- the consumer of the code indices: word x code counts ------------------------------------------------------------------
 * Replaces the per-token Python walk of analyses/unsupervised_vq_disentanglement/unsupervised_vq_disentanglement.py:166-200
 * (`vq_words_distrib[code].append(word)`, `seen_v_is.add(code)` for every token of every word :181-183;
 *  `words_of_interest_vq_distrib[word].append(v_is[0])` for a word's first token :192-199); the result files (:208-235) only use
 * counts and sets of those lists, i.e. projections of
 *     counts_all  [G][W][K] (uint32) += 1 for every token n with a word,      cell (g, slot(n), idx[n][g])
 *     counts_first[G][W][K] (uint32) += 1 for the FIRST token of every word,  same cell
 * slot_first [N] int32: -1 = the position belongs to no word (padding), else (slot << 1) | (1 if the word's first token);
 * idx [N][G] int64 = min_encoding_indices as the quantisers return them.  The tables ACCUMULATE (zero them before the first batch).
 * Positions with slot >= W or an index outside [0, K) are skipped and counted in *n_bad (optional).  Exact integer arithmetic;
 * G * W * K < 2^31. */
int kvq_code_census(const int32_t* slot_first, const int64_t* idx, int64_t N, int G, int K, int W, uint32_t* counts_all,
                    uint32_t* counts_first, uint32_t* n_bad, void* stream);


/* ---- latent analyses: group means of encoder outputs, the shift along their difference, the codebook gather -------------------
 * What analyses/latent_arithmetics/latent_arithmetics_Bagon.py:77-139 (v = mean enc(A) - mean enc(B); decode enc(C) + v) and
 * analyses/latent_traversals/latent_traversals_Shelgon_latent_classes.py:113-161 (overwrite the discrete latent, decode) do on the
 * host with every encoder output kept.  csrc/kvq_latent.hip.  Kernels only: capturable.  Activations are io_dtype (f32 / bf16)
 * [B, S, H] with a row stride in ELEMENTS between consecutive (b, s) rows; 16-byte accesses where base and stride allow them.
 *
 * kvq_latent_group_sum: table [G, S, H] f64 += the sum of x[b] over the sentences b with group[b] == g, count [G] int64 += their
 *   number.  group [B] int32: -1 = skip the sentence; a value >= G or < -1 is skipped and counted in *n_bad (optional).
 *   Deterministic, no floating-point atomics: a workgroup owns a contiguous run of sentences and a span of (s, h), adds the run in
 *   ascending sentence order in f64 registers and leaves a slab in ws; a second launch adds the slabs in ascending order into table.
 *   The same inputs give the same bits.  ws: kvq_latent_group_sum_workspace_bytes(B, S, H, G), 16-byte aligned; table 16-byte aligned.
 * kvq_latent_shift: out[b, s, :] = io(f32(x[b, s, :] + alpha * (table[g1, s, :] / count[g1] - table[g0, s, :] / count[g0]))) where
 *   sel[b, s] != 0 (sel [B, S] int8, NULL = every position), the bits of x elsewhere.  f64 arithmetic, each operation rounded on
 *   its own, then round-to-nearest-even to f32 and to io_dtype.  The counts are read on the device; a group with count 0 means
 *   "no shift" (out = x).  out may be x.
 * kvq_vq_lookup: out[n, g * Dg : (g + 1) * Dg] = io(E[g][idx[n][g]]) for idx [N, G] int64 and the f32 codebooks E [G, K, Dg] -- the
 *   quantiser's gather without its distances: the codebook row itself, not the straight-through value fl(z + fl(e - z)).  An index
 *   outside [0, K) leaves a zero row and is counted in *n_bad (optional). */
size_t kvq_latent_group_sum_workspace_bytes(int64_t B, int S, int H, int G);
int kvq_latent_group_sum(const void* x, int64_t ldx, const int32_t* group, int64_t B, int S, int H, int G, int io_dtype, double* table,
                         int64_t* count, uint32_t* n_bad, void* ws, size_t ws_bytes, void* stream);
int kvq_latent_shift(const void* x, int64_t ldx, const double* table, const int64_t* count, int g1, int g0, double alpha,
                     const int8_t* sel, int64_t B, int S, int H, int G, int io_dtype, void* out, int64_t ldo, void* stream);
int kvq_vq_lookup(const int64_t* idx, const float* E, int64_t N, int K, int Dg, int G, int io_dtype, void* out, int64_t ldo,
                  uint32_t* n_bad, void* stream);


/* Word-embedding gradient (autograd of the row gather of BertEmbeddings, modeling_bert.py:53-58):
 *     gW[id][:] (= | +=) sum over the tokens n with ids[n] == id of g[n][:],   tokens added in increasing n  (deterministic)
 * The caller passes the tokens sorted by id: sorted_ids[s] ascending and perm[s] = the token at sorted position s (a STABLE
 * sort, e.g. torch.sort(ids, stable=True)); the same pair serves every embedding table looked up with these ids.
 * g [N, H] (g_dtype), gW [V, H] (w_dtype); with accumulate == 0 only the rows of ids that occur are written (zero gW first),
 * ids outside [0, V) are ignored.  H %% 4 == 0, H <= 1024.  No float atomics. */
size_t kvq_embed_grad_workspace_bytes(int64_t N, int H);
int kvq_embed_grad(const void* g, const int64_t* perm, const int64_t* sorted_ids, int64_t N, int H, int64_t V, int g_dtype,
                   void* gW, int w_dtype, int accumulate, void* ws, size_t ws_bytes, void* stream);


/* One Lloyd iteration's centroid update (the data-driven codebook initialiser of the reference runs
 * scipy.cluster.vq.kmeans2(z, K, minit='points') on encoder outputs, models/shelgon3/vq_codebook_init_weights.py:85-101):
 *     E_k <- mean of the rows z_n with idx_n == k  (f64 accumulation of per-chunk f32 sums, rows added in increasing n);
 *     a cluster without rows keeps its centroid (kmeans2's missing='warn');  counts[K] (may be NULL) receives the cluster sizes.
 * The assignment step of the iteration IS the hot kernel: kvq_vq_forward(z, E) -> idx.  ws: kvq_vq_workspace_bytes(N,K,D,1). */
int kvq_kmeans_update(const void* z, const int64_t* idx, int64_t N, int K, int D, int io_dtype, float* E, int64_t* counts,
                      void* ws, size_t ws_bytes, void* stream);


/* ---- Gumbel-softmax quantiser (the reference's other VQ_MODE, models/shelgon3/GumbelQuantizer.py:43-83) ---------------------
 * Row-wise part of GumbelQuantizer.forward between its two GEMMs (logits = proj(z), z_q = y . embed):
 *   y_soft = softmax((logits + g) / tau) with g ~ Gumbel(0,1);  ind = argmax(y_soft) (first maximum);
 *   y = y_soft, or (hard != 0) fl(fl(one_hot(ind) - y_soft) + y_soft): torch.nn.functional.gumbel_softmax's return value;
 *   kl_row[n] = sum_k q log(q K + 1e-10), q = softmax(logits)   (diff = kld_scale * mean_n kl_row, :73).
 * logits, y [N,K] io_dtype; y_soft [N,K] f32 (kept for backward; may be NULL), ind [N] int64, kl_row [N] f32.
 * noise [N,K] f32 supplies g explicitly (parity tests against torch's generator); NULL draws it from Philox4x32-10
 * (seed, site; plus the device step count when kvq_set_seed_offset is active).  K <= 1024.
 * Backward: g_logits = y_soft (g_y - <y_soft,g_y>) / tau  +  g_diff kld_scale/N * q (L - <q,L>),
 *   L = log(q K + 1e-10) + q K / (q K + 1e-10); g_y may be NULL (no gradient through y), g_diff NULL means 1. */
int kvq_gumbel_forward(const void* logits, const float* noise, int64_t N, int K, float tau, int hard, uint64_t seed, uint32_t site,
                       int io_dtype, void* y, float* y_soft, int64_t* ind, float* kl_row, void* stream);
int kvq_gumbel_backward(const void* logits, const float* y_soft, const void* g_y, const float* g_diff, int64_t N, int K, float tau,
                        float kld_scale, int io_dtype, void* g_logits, void* stream);


/* ---- free-running generation: one decoder token per sentence and launch, over a key/value cache (csrc/kvq_generate.hip) --------
 * What the teacher-forced decoder call (models/bagon/Bagon.py:46-53, models/shelgon3/Shelgon.py:71) cannot answer: the sentence a
 * latent produces when the decoder sees only what it has written itself.  DESIGN.md section 5i.
 *
 * Generation state, on the device (the pattern of the accumulation state): 32 bytes, 8-byte aligned,
 *     struct { int32 t, P, Lmax, eos_id, pad_id; uint32 seed_lo, seed_hi; float inv_tau; }
 *   t = the position being decoded (the token at column t of `ids` is the step's input), P = prompt length (columns 0 .. P-1 of
 *   `ids` are given), Lmax = columns of `ids`, eos_id < 0 = no end token; seed = the 64-bit Philox key of the sampling draws,
 *   inv_tau = 1 / temperature, 0 = greedy.  Beside it ids [B, Lmax] int64, finished [B] int32,
 *   lengths [B] int32.  EVERY kernel below reads t from the state, never from a launch argument: one captured step serves every
 *   position.  Kernels only, no floating-point atomics (no atomics at all), the same inputs give the same bits; f32 and bf16 io.
 *   A state whose t lies outside what the buffers hold (t >= Lmax, t >= pos_rows, t >= Smax) makes the kernels store nothing.
 *
 * kvq_gen_embed   BertEmbeddings (modeling_bert.py:53-110) of one token per sentence at evaluation:
 *                     out[b, :] = LayerNorm(word[ids[b, t]] + (pos[t] + type_row))            out [B, H] io dtype
 *                 with the arithmetic, roundings and summation order of kvq_embed_ln_fwd (p_drop = 0): the bits of its row for the
 *                 same token at the same position.  pos has pos_rows rows.  H %% 4 == 0, H <= 4096.
 * kvq_gen_attn    BertSelfAttention / cross-attention core (:111-204) for ONE query row per (sentence, head), head dim 64:
 *                     out[b, h*64 ..] = softmax(q[b, h] . K[b, :n, h]^T * 1/8) . V[b, :n, h]
 *                 q [B, ldq], out [B, ldo]; kv: keys at column h*64, values at column nh*64 + h*64 of row j of sentence b, at
 *                 kv + b * kv_sentence_stride + j * ld_kv (elements).
 *                   append != 0 (self-attention): k_new / v_new [B, ld_new] are this step's rows (column slices of the fused q|k|v
 *                     projection); the kernel stores them to row t of the cache kv [B, Smax, 2 nh 64] and attends over rows 0 .. t
 *                     (n = t + 1, n_keys is ignored).  A workgroup owns one (sentence, head) and touches only that head's columns.
 *                   append == 0 (cross-attention): n = n_keys, 1 .. 128; kv is a layer's column slice of the projected latent
 *                     (ld_kv = the row stride of that buffer); k_new, v_new are ignored.  No mask.
 *                 Scores and probabilities f32, the output rounded once to the io dtype.  16-byte accesses: every pointer 16-byte
 *                 aligned, every stride a multiple of 16 bytes.  Smax <= 128.
 * kvq_gen_select  the next token of every sentence from logits [B, ld] io dtype (columns >= V never win), one workgroup a sentence:
 *                     choice = first arg-max over v < V of (logit_v * inv_tau + g_v); a NaN never wins (a row of NaNs chooses 0)
 *                   inv_tau and seed are read from the state, as t is: the same launch serves every temperature and seed.
 *                   state.inv_tau == 0: g = 0 and inv_tau = 1 (greedy).  Otherwise g_v = -log(-log u), u from
 *                     philox4x32(c0 = v / 4, c1 = b, c2 = t, c3 = 0x47454e53; key = seed) word v %% 4, u = ((bits >> 9) + 0.5) 2^-23,
 *                     which is exact in f32 and inside [2^-24, 1 - 2^-24], so g is finite for every bit pattern: the Gumbel-max
 *                     trick, a draw from softmax(logits * inv_tau) (on a grid of 2^23 uniforms).
 *                     kvq_gen_gumbel_debug (test hook): out[i] = g of bits[i] as the kernel forms it.
 *                   then, when t + 1 < Lmax:  t + 1 < P: ids[b, t+1] is kept (prompt);  else finished[b]: ids[b, t+1] = pad_id;
 *                     else ids[b, t+1] = choice and, if choice == eos_id, finished[b] = 1 and lengths[b] = t + 2.
 *                   step_logits (may be NULL) [B, Lmax, V] f32: row (b, t) receives the logits of columns < V.
 *                 ld %% 8 == 0, 16-byte aligned logits.
 * kvq_gen_select_filtered  kvq_gen_select on a top-k / top-p filtered distribution, with the score of what it chose (DESIGN.md
 *                 section 5k).  Filter state, on the device beside the generation state: 16 bytes, 4-byte aligned,
 *                     struct { int32 top_k; float top_p; int32 reserved[2]; }
 *                   reserved = 0; a non-zero reserved word makes the kernel store nothing.  The filters are read from there, never
 *                   from a launch argument: one captured step serves every (top_k, top_p, temperature, seed).
 *                   y_v = fl32(logit_v * inv_tau) for v < V, the product of kvq_gen_select (inv_tau = 1 and g = 0 in a greedy state).
 *                   A NaN is never kept and never counted (n_valid = the others); a -inf has mass 0.
 *                   ORDER: v before w iff y_v > y_w, or y_v == y_w and v < w.  Every kept set is a prefix of the order.
 *                   top-k (top_k >= 1): K = the first min(top_k, n_valid) of the order; top_k <= 0: K = every valid column.
 *                   top-p (0 < top_p < 1; anything else, a NaN included, turns it off), inside K as HuggingFace chains its warpers:
 *                     m = max y, e_v = exp(y_v - m), Z = sum over K of e, C_j = the mass of the first j of the order;
 *                     n_keep = the smallest j >= 1 with C_j >= fl(top_p Z) -- the token that crosses p is kept
 *                     (TopPLogitsWarper) -- and |K| if no j reaches it in the kernel's arithmetic.
 *                   choice = the first arg-max over the kept set of (y_v + g_v), g_v EXACTLY kvq_gen_select's noise (same Philox
 *                     counters, key and u -> g): filters off, the bits of kvq_gen_select; filters on, kvq_gen_select on the logits
 *                     with every column outside the kept set at -inf.  An exact draw from the distribution renormalised over the set.
 *                   A greedy state ignores the filters (the arg-max is in every kept set): n_keep = n_valid.  A row with no valid
 *                   logit chooses 0 with n_keep = 0.  Prompt / finished / end-token bookkeeping and step_logits: kvq_gen_select's.
 *                   step_kept, step_cut [B, Lmax] int32, step_logprob [B, Lmax] f32 (each may be NULL): row (b, t) receives n_keep,
 *                     the id of the last kept element of the order (-1 when n_keep = 0) and
 *                     log p~(choice) = fl(fl(y_c - m) - log C_n_keep), p~ = the distribution that was sampled from (NaN when n_keep = 0).
 *                   One workgroup of 1024 threads a sentence, the row read once (16 bytes a lane) and held in registers:
 *                   V <= 32768, refused above.  The cut is a selection, not a sort: y maps to an order-preserving 32-bit key and the
 *                   key of the last kept element is found bit by bit, one block reduction (count and mass of the keys continuing
 *                   the decided prefix with a 1) a bit; the group tied at the cut shares one mass e_T, so the j of it to keep follow
 *                   from the count / mass left, and the cut is its j-th lowest index (a 16-bit selection of the same kind).
 *                   No atomics, fixed summation orders: the same inputs give the same bits, eagerly and under graph replay.
 *                   ROUNDING.  A mass is summed as: 8 columns of a thread as a tree (3 roundings), its 4 chunks in order (3), the
 *                   wave as a butterfly (6), the 16 waves as a tree (4) = 16; C_j adds at most 32 such sums in the order of the
 *                   rounds (32) and j e_T (2): 50 roundings, each at most 2^-24 of a partial sum <= Z.  A term e_v carries the
 *                   rounding of y_v - m (2^-24 |y_v - m| relative; summed with weights e_v / Z that is at most 2^-24 log V <= 10.4
 *                   2^-24, the entropy bound) and expf's 1 ulp (2 2^-24).  So |C_j - exact| <= 62.4 2^-24 Z, the same for Z, one
 *                   more rounding for top_p Z: the comparison C_j >= top_p Z is decided as an exact one at some p' with
 *                       |p' - top_p| <= TOL_MASS = 2^-17     (>= (2 * 62.4 + 1) 2^-24)
 *                   and  |step_logprob - exact| <= 2^-17 + 2^-22 (|y_c - m| + |log C|)   (log C: C's relative error 62.4 2^-24 <
 *                   2^-18 by the same count relative to C >= 1, logf's ulp and two subtractions on top).  tests/_sample_ref.py.
 *                 ld %% 8 == 0, 16-byte aligned logits.
 * kvq_gen_advance one thread: t += 1.  A launch of its own, so that no kernel of a step races with the increment. */
int kvq_gen_embed(const void* state, const int64_t* ids, const void* word, const void* pos, const void* type_row, const float* gamma,
                  const float* beta, int B, int H, int64_t V, int pos_rows, float eps, int io_dtype, void* out, void* stream);
int kvq_gen_attn(const void* state, const void* q, int64_t ldq, const void* k_new, const void* v_new, int64_t ld_new, void* kv,
                 int64_t ld_kv, int64_t kv_sentence_stride, int B, int nh, int append, int n_keys, int Smax, int io_dtype, void* out,
                 int64_t ldo, void* stream);
int kvq_gen_select(const void* state, const void* logits, int64_t ld, int V, int B, int io_dtype, int64_t* ids, int32_t* finished,
                   int32_t* lengths, float* step_logits, void* stream);
int kvq_gen_select_filtered(const void* state, const void* filter, const void* logits, int64_t ld, int V, int B, int io_dtype, int64_t* ids,
                            int32_t* finished, int32_t* lengths, float* step_logits, int32_t* step_kept, int32_t* step_cut,
                            float* step_logprob, void* stream);
int kvq_gen_gumbel_debug(const uint32_t* bits, int64_t n, float* out, void* stream);
int kvq_gen_advance(void* state, void* stream);


/* ---- beam search over the key/value cache (csrc/kvq_generate.hip) ------------------------------------------
 * Slot space: beam w of sentence b is row r = b W + w of every [R, ...] buffer, R >= B W (the engine rounds it up to 8; a last
 * sentence with fewer than W rows is handled).  Nothing is ever moved: row (r, t) of a cache and ids[r, t] are written once, by
 * row r at position t, and a beam's HISTORY is a row of the ancestry table
 *     anc [2, R, Lmax] int32, ping-ponged on the parity of t:  anc[t & 1][r, j], j <= t  =  the slot whose cache row j and token j
 *     belong to the history of the beam now living in row r          (both halves start as the identity, anc[., r, j] = r)
 * beside ids [R, Lmax] int64 (slot tokens: kvq_gen_embed and kvq_gen_advance run on it unchanged), parent [R, Lmax] int32,
 * step_scores [R, Lmax] f32, scores [R] f32 (sums of log-probabilities; -inf = a dead beam, which offers nothing), finished [R],
 * lengths [R] int32.  The state is the generation state above with inv_tau = 0, seed = 0; every kernel reads t from it.  Kernels
 * only, no atomics, fixed summation orders: the same inputs give the same bits.  f32 and bf16 io.
 *
 * kvq_beam_attn    kvq_gen_attn with two indirections in the addresses; arithmetic, lane mapping and summation order are that
 *                  kernel's (one body): on a cache gathered physically by the same ancestry the two agree bit for bit.
 *                    append != 0: row r stores its k_new | v_new to cache row (r, t) and attends over keys j = 0 .. t, key j < t read
 *                      from cache row (anc[t & 1][r, j], j), key t from k_new / v_new themselves (no workgroup waits for another's
 *                      store).  anc_ld = Lmax >= Smax.  A slot outside [0, R) reads row r.
 *                    append == 0: row r reads the n_keys rows of sentence r / rows_per_sentence of kv.
 * kvq_beam_select  one step of the search, one workgroup a sentence (rows b W .. b W + W - 1, W = 1 .. 8, W <= V); everything of
 *                  the old state is read before anything is written.  Stores nothing unless 0 <= t and t + 1 < Lmax.
 *                    t + 1 < P (prompt): ids kept, parent[r, t+1] = r, step_scores[r, t+1] = scores[r], the history extended by
 *                      anc'[r, 0 .. t] = anc[r, 0 .. t], anc'[r, t+1] = r      (anc = half t & 1, anc' = half (t + 1) & 1).
 *                    otherwise the candidates are: of a live beam w (not finished, score > -inf) every v < V with
 *                        lp = fl(x[w, v] - lse_w),  s = fl(score_w + lp),  lse_w = m + log sum_v exp(x[w, v] - m)   (f32)
 *                      -- a beam with a NaN among its columns < V offers nothing, a candidate with s = -inf or NaN is none --;
 *                      of a finished beam exactly one: token pad_id, s = score_w, ranking in ties as (w, 0).  New beam i = the i-th
 *                      best: larger s, then lower w, then lower v.  For the new row r' = b W + i with parent w:
 *                        ids[r', t+1] = v, parent[r', t+1] = b W + w, scores[r'] = step_scores[r', t+1] = s, finished / lengths of w,
 *                        v == eos_id: finished = 1, lengths = t + 2;  anc'[r', 0 .. t] = anc[b W + w, 0 .. t], anc'[r', t+1] = r'.
 *                      Fewer than W candidates: the rest become dead beams (score -inf, token pad_id, parent = self, finished = 1,
 *                      their own history).
 *                    The logits are read once, 16 bytes a lane; the chain of f32 roundings in front of lse_w is bounded by 256
 *                    (refused otherwise: V up to 55 296 with 5 .. 8 beams, 106 496 with 3 or 4, more with fewer), which is what the tolerance of tests/_beam_ref.py rests on.
 *                    step_logits (may be NULL) [R, Lmax, V] f32: row (r, t) receives the logits of every row in the prompt, of
 *                    the live beams afterwards.  ld %% 8 == 0, 16-byte aligned logits.
 * kvq_beam_gather  hypotheses from slot space: out[r, j] = ids[anc[t & 1][r, j], j] for j < lengths[r] (j <= t), pad_id behind. */
int kvq_beam_attn(const void* state, const void* q, int64_t ldq, const void* k_new, const void* v_new, int64_t ld_new, void* kv,
                  int64_t ld_kv, int64_t kv_sentence_stride, int R, int nh, int append, int n_keys, int Smax, const int32_t* anc,
                  int anc_ld, int rows_per_sentence, int io_dtype, void* out, int64_t ldo, void* stream);
int kvq_beam_select(const void* state, const void* logits, int64_t ld, int V, int R, int W, int Lmax, int io_dtype, int64_t* ids,
                    int32_t* parent, float* scores, float* step_scores, int32_t* anc, int32_t* finished, int32_t* lengths,
                    float* step_logits, void* stream);
int kvq_beam_gather(const void* state, const int64_t* ids, const int32_t* anc, const int32_t* lengths, int R, int Lmax, int64_t* out,
                    void* stream);


/* ---- free-running reconstruction metrics (csrc/kvq_seqcmp.hip) ---------------------------------------------
 * What a generated sentence has to do with the sentence it should have been: token edit distance, positional matches, lengths.
 * Teacher-forced accuracy (kvq_seq_acc) hands the decoder the true prefix at every position and cannot see a dropped or inserted
 * word; these kernels compare what kvq_gen_select / kvq_beam_gather wrote with a reference, on the device.  Integers only: the same
 * inputs give the same bits in any order of execution.  Neither kernel is part of the captured training step.
 *
 * kvq_seq_compare  per sentence b:
 *                    hypothesis h = hyp[b, hyp_skip .. hyp_len[b] - 1], n = hyp_len[b] - hyp_skip tokens (hyp_len: the `lengths` of
 *                      generation, prompt included; hyp_skip: the prompt length); reference r = ref[b, 0 .. ref_len[b] - 1], m tokens;
 *                    out[b] = (dist, hits, n, m), int32:
 *                      dist = the Levenshtein distance of h and r, insertion, deletion and substitution at cost 1 each
 *                             (n == 0 or m == 0: max(n, m)); the pair is an exact match iff dist == 0;
 *                      hits = #{j < min(n, m) : h[j] == r[j]}.
 *                    Tokens are compared on all 64 bits.  0 <= n, m <= Lmax <= 128 (refused above: the launcher knows Lmax only).
 *                    A row whose lengths on the device lie outside that range -- or past its row: hyp_len[b] > ld_hyp, ref_len[b] >
 *                    ld_ref -- is not read: out[b] = (-1, 0, 0, 0) and *n_bad += 1 (n_bad: int64 on the device, the caller zeroes
 *                    it; the pattern of kvq_latent_group_sum).  The other rows are unaffected.
 *                    One wavefront per pair, four per workgroup; the DP table is walked by anti-diagonals, a lane owning reference
 *                    columns l + 1 and l + 65 with the last two diagonals in registers and the hypothesis in LDS.  No global
 *                    scratch; the only atomic is the one on n_bad.  out 16-byte aligned.
 * kvq_seq_compare_accumulate  for every sentence with dist >= 0 and every column c with 0 <= slot[b, c] < R:
 *                        table[slot[b, c]] += (1, dist == 0, dist, hits, n, m)            table [R, 6] int64, slot [B, C] int32
 *                    A slot outside [0, R) is skipped, as is a sentence kvq_seq_compare marked with dist = -1.  64-bit integer
 *                    atomics: exact, order-free.  One launch, no host read.  R <= 4096, C <= 16; per 16-byte aligned. */
int kvq_seq_compare(const int64_t* hyp, int64_t ld_hyp, int hyp_skip, const int32_t* hyp_len, const int64_t* ref, int64_t ld_ref,
                    const int32_t* ref_len, int64_t B, int Lmax, int32_t* out, int64_t* n_bad, void* stream);
int kvq_seq_compare_accumulate(const int32_t* per, int64_t B, const int32_t* slot, int C, int64_t R, int64_t* table, void* stream);


#ifdef __cplusplus
}
#endif
#endif /* KVQ_H */
