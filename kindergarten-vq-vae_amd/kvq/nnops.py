"""Tensor-level wrappers of the fused block kernels in libkvq.so (csrc/kvq_nn.hip, csrc/kvq_ln.hip).  Plain functions, no autograd:
the training engine (kvq/engine.py) calls forward and backward kernels explicitly.  All work goes to the current stream."""
from __future__ import annotations

import torch

from ._ffi import FP8_E4M3, FP8_E5M2, KvqError, check, io_dtype_of, lib, require_gpu, stream_ptr
from .functional import _workspace


def _p(t):
    return None if t is None else t.data_ptr()


def ln_fwd(y, resid, gamma, beta, eps, p_drop=0.0, seed=0, site=0, save_pre=True):
    """out = LayerNorm(dropout(y) + resid).  Returns (out, pre, mean, rstd); pre = the LN input as stored."""
    require_gpu(y, gamma, beta)
    N, H = y.shape
    out = torch.empty_like(y)
    pre = torch.empty_like(y) if save_pre else None
    mean = torch.empty(N, dtype=torch.float32, device=y.device)
    rstd = torch.empty(N, dtype=torch.float32, device=y.device)
    check(lib().kvq_dropout_residual_ln_fwd(y.data_ptr(), _p(resid), gamma.data_ptr(), beta.data_ptr(), N, H, float(eps),
                                            float(p_drop), int(seed), int(site), io_dtype_of(y), out.data_ptr(), _p(pre),
                                            mean.data_ptr(), rstd.data_ptr(), stream_ptr()), "kvq_dropout_residual_ln_fwd")
    return out, pre, mean, rstd


def ln_fwd_fp8(y, resid, gamma, beta, eps, p_drop, seed, site, state, save_pre=True):
    """ln_fwd plus the fp8 (e4m3) copy of `out` for the fp8 GEMM that reads it next: (out, pre, mean, rstd, out8).  out8 holds the
    bytes kvq_fp8_quantize_delayed(out, state) would write; the call's amax is noted in `state` (one delayed-scaling record)."""
    require_gpu(y, gamma, beta)
    N, H = y.shape
    assert y.dtype == torch.bfloat16
    out = torch.empty_like(y)
    out8 = torch.empty((N, H), dtype=torch.uint8, device=y.device)
    pre = torch.empty_like(y) if save_pre else None
    mean = torch.empty(N, dtype=torch.float32, device=y.device)
    rstd = torch.empty(N, dtype=torch.float32, device=y.device)
    check(lib().kvq_dropout_residual_ln_fwd_fp8(y.data_ptr(), _p(resid), gamma.data_ptr(), beta.data_ptr(), N, H, float(eps),
                                                float(p_drop), int(seed), int(site), out.data_ptr(), _p(pre), mean.data_ptr(),
                                                rstd.data_ptr(), out8.data_ptr(), state.data_ptr(), stream_ptr()),
          "kvq_dropout_residual_ln_fwd_fp8")
    return out, pre, mean, rstd, out8


def ln_bwd(g_out, pre, mean, rstd, gamma, p_drop=0.0, seed=0, site=0, g_gamma=None, g_beta=None, accumulate=False,
           need_g_y=True, need_g_resid=True, g_bias_prev=None):
    """Returns (g_y, g_resid).  g_gamma / g_beta (f32 or bf16 [H]) are written (or accumulated into) when given;
    g_bias_prev receives colsum(g_y) = the bias gradient of the dense layer in front of this block."""
    N, H = g_out.shape
    g_y = torch.empty_like(g_out) if need_g_y else None
    g_resid = torch.empty_like(g_out) if need_g_resid else None
    l = lib()
    ws = _workspace(g_out.device, l.kvq_ln_bwd_workspace_bytes(N, H))
    ref = g_gamma if g_gamma is not None else (g_beta if g_beta is not None else g_bias_prev)
    pdt = io_dtype_of(ref) if ref is not None else 0
    check(l.kvq_dropout_residual_ln_bwd(g_out.data_ptr(), pre.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), N, H,
                                        float(p_drop), int(seed), int(site), io_dtype_of(g_out), _p(g_y), _p(g_resid), _p(g_gamma),
                                        _p(g_beta), _p(g_bias_prev), pdt, int(accumulate), ws.data_ptr(), ws.numel(), stream_ptr()),
          "kvq_dropout_residual_ln_bwd")
    return g_y, g_resid


def colsum(x, out, scale=1.0, accumulate=False, cols=None):
    """out[c] (= | +=) scale * sum_n x[n, c] for the first `cols` columns of a row-major 2-D tensor (row stride = x.stride(0))."""
    N = x.shape[0]
    C = x.shape[1] if cols is None else cols
    l = lib()
    ws = _workspace(x.device, l.kvq_colsum_workspace_bytes(N, C))
    check(l.kvq_colsum(x.data_ptr(), N, C, x.stride(0), io_dtype_of(x), out.data_ptr(), io_dtype_of(out), float(scale),
                       int(accumulate), ws.data_ptr(), ws.numel(), stream_ptr()), "kvq_colsum")
    return out


def ln_bwd_partial(g_out, pre, mean, rstd, gamma, p_drop=0.0, seed=0, site=0, need_g_y=True, need_g_resid=True, want_dbias=False):
    """LayerNorm backward without the final parameter-gradient sums: returns (g_y, g_resid, part) with part [rows, 3H] f32 =
    per-workgroup partials [dbias_prev | dgamma | dbeta]; hand column ranges of `part` to reduce_batch()."""
    N, H = g_out.shape
    g_y = torch.empty_like(g_out) if need_g_y else None
    g_resid = torch.empty_like(g_out) if need_g_resid else None
    l = lib()
    part = torch.empty((l.kvq_ln_bwd_partial_rows(N), 3 * H), dtype=torch.float32, device=g_out.device)
    check(l.kvq_dropout_residual_ln_bwd_partial(g_out.data_ptr(), pre.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                N, H, float(p_drop), int(seed), int(site), io_dtype_of(g_out), _p(g_y), _p(g_resid),
                                                int(want_dbias), part.data_ptr(), part.numel() * 4, stream_ptr()),
          "kvq_dropout_residual_ln_bwd_partial")
    return g_y, g_resid, part


def embed_ln_fwd(ids, word, pos, type_row, gamma, beta, eps, seq_len, p_drop=0.0, seed=0, site=0):
    """BertEmbeddings in one kernel: out = dropout(LayerNorm(word[ids] + pos[n % seq_len] + type_row)).
    Returns (out, pre, mean, rstd) like ln_fwd; ids flat int64 [N]."""
    require_gpu(ids, word, pos)
    N, H = ids.numel(), word.shape[1]
    if pos.shape[0] < seq_len or N % seq_len != 0:      # the kernel reads pos[(n % seq_len)]: rows that must exist
        raise KvqError(f"kvq.nnops.embed_ln_fwd: {N} ids in sentences of {seq_len} tokens need {seq_len} position rows "
                       f"(the table has {pos.shape[0]}) and a whole number of sentences")
    out = torch.empty((N, H), dtype=word.dtype, device=word.device)
    pre = torch.empty_like(out)
    mean = torch.empty(N, dtype=torch.float32, device=word.device)
    rstd = torch.empty(N, dtype=torch.float32, device=word.device)
    check(lib().kvq_embed_ln_fwd(ids.data_ptr(), word.data_ptr(), pos.data_ptr(), type_row.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                 N, int(seq_len), H, word.shape[0], float(eps), float(p_drop), int(seed), int(site), io_dtype_of(word),
                                 out.data_ptr(), pre.data_ptr(), mean.data_ptr(), rstd.data_ptr(), stream_ptr()), "kvq_embed_ln_fwd")
    return out, pre, mean, rstd


def ln_dropout_bwd_partial(g_out, pre, mean, rstd, gamma, p_drop, seed, site):
    """Backward of dropout(LayerNorm(x)) (the embedding block): returns (g_x, part) with part [rows, 3H] f32 = [- | dgamma | dbeta]."""
    N, H = g_out.shape
    g_x = torch.empty_like(g_out)
    l = lib()
    part = torch.empty((l.kvq_ln_bwd_partial_rows(N), 3 * H), dtype=torch.float32, device=g_out.device)
    check(l.kvq_ln_dropout_bwd_partial(g_out.data_ptr(), pre.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), N, H,
                                       float(p_drop), int(seed), int(site), io_dtype_of(g_out), g_x.data_ptr(), part.data_ptr(),
                                       part.numel() * 4, stream_ptr()), "kvq_ln_dropout_bwd_partial")
    return g_x, part


def colsum_partial(x, cols=None):
    """Per-workgroup partial column sums of a row-major 2-D tensor: part [rows, C] f32 (finish with reduce_batch())."""
    N = x.shape[0]
    C = x.shape[1] if cols is None else cols
    l = lib()
    part = torch.empty((l.kvq_colsum_partial_rows(N), C), dtype=torch.float32, device=x.device)
    check(l.kvq_colsum_partial(x.data_ptr(), N, C, x.stride(0), io_dtype_of(x), part.data_ptr(), part.numel() * 4, stream_ptr()),
          "kvq_colsum_partial")
    return part


def reduce_item(src, dst, count, cols, ld, scale=1.0, accumulate=False, src_offset=0):
    """One entry of reduce_batch(): dst[c] (= | +=) scale * sum_{p<count} src.flat[src_offset + p*ld + c], c < cols."""
    from ._ffi import ReduceItem
    return ReduceItem(src.data_ptr() + src_offset * src.element_size(), dst.data_ptr(), int(count), int(cols), int(ld), float(scale),
                      io_dtype_of(src), io_dtype_of(dst), int(accumulate))


def reduce_batch(items):
    """Run a list of reduce_item()s, KVQ_REDUCE_MAX_ITEMS per launch.  The caller keeps the source tensors alive until here."""
    from ._ffi import ReduceItem, KVQ_REDUCE_MAX_ITEMS
    l = lib()
    st = stream_ptr()
    for i in range(0, len(items), KVQ_REDUCE_MAX_ITEMS):
        chunk = items[i:i + KVQ_REDUCE_MAX_ITEMS]
        arr = (ReduceItem * len(chunk))(*chunk)
        check(l.kvq_reduce_batch(arr, len(chunk), st), "kvq_reduce_batch")


def sum_slabs(part, out):
    """out = part.sum(0) for a [S, ...] stack of split-K partial results (f32 accumulate)."""
    S = part.shape[0]
    check(lib().kvq_sum_slabs(part.data_ptr(), S, out.numel(), io_dtype_of(part), out.data_ptr(), stream_ptr()), "kvq_sum_slabs")
    return out


def gelu_fwd(h):
    a = torch.empty_like(h)
    check(lib().kvq_gelu_fwd(h.data_ptr(), a.data_ptr(), h.numel(), io_dtype_of(h), stream_ptr()), "kvq_gelu_fwd")
    return a


def gelu_bwd(h, g_a, out=None):
    g_h = torch.empty_like(h) if out is None else out
    check(lib().kvq_gelu_bwd(h.data_ptr(), g_a.data_ptr(), g_h.data_ptr(), h.numel(), io_dtype_of(h), stream_ptr()), "kvq_gelu_bwd")
    return g_h


def gelu_bwd_bias(h, g_a, out=None):
    """(g_h, part): gelu_bwd plus part [rows, C] f32 partial column sums of g_h (bias gradient partials for reduce_batch())."""
    N, Cc = h.shape
    g_h = torch.empty_like(h) if out is None else out
    l = lib()
    part = torch.empty((l.kvq_gelu_bwd_partial_rows(N), Cc), dtype=torch.float32, device=h.device)
    check(l.kvq_gelu_bwd_bias(h.data_ptr(), g_a.data_ptr(), g_h.data_ptr(), N, Cc, io_dtype_of(h), part.data_ptr(), part.numel() * 4,
                              stream_ptr()), "kvq_gelu_bwd_bias")
    return g_h, part


def attn_fwd(q, k, v, mask, B, nh, Sq, Sk, causal, p_drop=0.0, seed=0, site=0, out=None):
    """q [B*Sq, >=nh*64] (any row stride), k, v [B*Sk, ...]; returns (ctx [B*Sq, nh*64], lse [B, nh, Sq])."""
    require_gpu(q, k, v)
    dh = 64
    ctx = torch.empty((B * Sq, nh * dh), dtype=q.dtype, device=q.device) if out is None else out
    lse = torch.empty((B, nh, Sq), dtype=torch.float32, device=q.device)
    check(lib().kvq_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), _p(mask), B, nh, Sq, Sk, dh, q.stride(0), k.stride(0),
                             v.stride(0), ctx.stride(0), int(causal), 1.0 / 8.0, float(p_drop), int(seed), int(site),
                             io_dtype_of(q), ctx.data_ptr(), lse.data_ptr(), stream_ptr()), "kvq_attn_fwd")
    return ctx, lse


def attn_probs(q, k, v, mask, B, nh, Sq, Sk, causal, lse=None, probs=None, table=None):
    """The softmax probabilities of attn_fwd's operands, without dropout (kvq_attn_probs): written to probs [B, nh, Sq, Sk] f32
    and / or summed over the B sentences INTO table [nh, Sq, Sk] f64 (contiguous, or a contiguous slice).  lse: attn_fwd's, needed
    above 32 tokens.  Returns probs."""
    require_gpu(q, k)
    for t, dt, shape in ((probs, torch.float32, (B, nh, Sq, Sk)), (table, torch.float64, (nh, Sq, Sk))):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous()):
            raise KvqError(f"attn_probs: output must be a contiguous {dt} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
    if lse is not None and (lse.dtype != torch.float32 or tuple(lse.shape) != (B, nh, Sq) or not lse.is_contiguous()):
        raise KvqError("attn_probs: lse must be attn_fwd's contiguous f32 [B, nh, Sq]")
    l = lib()
    ws, nws = None, 0
    if table is not None:
        nws = l.kvq_attn_probs_workspace_bytes(B, nh, Sq, Sk)
        ws = _workspace(q.device, nws)       # slabs: written and consumed inside this call, on this stream
    check(l.kvq_attn_probs(q.data_ptr(), k.data_ptr(), _p(v), _p(mask), _p(lse), B, nh, Sq, Sk, 64, q.stride(0), k.stride(0),
                           v.stride(0) if v is not None else 0, int(causal), 1.0 / 8.0, io_dtype_of(q), _p(probs), _p(table), _p(ws), nws,
                           stream_ptr()), "kvq_attn_probs")
    return probs


def _rows3(x, what):
    """(B, S, H, row stride in elements) of an activation [B, S, H] whose (b, s) rows lie at one stride (a contiguous tensor, or a
    column slice of one)."""
    if x.dim() != 3 or x.stride(2) != 1 or (x.shape[0] > 1 and x.stride(0) != x.shape[1] * x.stride(1)):
        raise KvqError(f"{what}: needs [B, S, H] activations with unit column stride and evenly strided rows, got shape "
                       f"{tuple(x.shape)} strides {tuple(x.stride())}")
    B, S, H = x.shape
    return B, S, H, (x.stride(1) if S > 1 else max(x.stride(0), H))


def latent_group_sum(x, group, table, count, n_bad=None):
    """table [G, S, H] f64 += per-group sums of x [B, S, H] (f32 / bf16), count [G] int64 += sentences per group
    (kvq_latent_group_sum).  group [B] int32: -1 skips a sentence; labels outside [-1, G) are skipped and counted in n_bad
    ([1] int32, optional).  Deterministic: no float atomics."""
    require_gpu(x, group, table, count, n_bad)
    B, S, H, ldx = _rows3(x, "latent_group_sum")
    G = table.shape[0] if table.dim() == 3 else -1
    if table.dtype != torch.float64 or tuple(table.shape) != (G, S, H) or not table.is_contiguous():
        raise KvqError(f"latent_group_sum: table must be a contiguous float64 [G, {S}, {H}], got {table.dtype} {tuple(table.shape)}")
    if count.dtype != torch.int64 or tuple(count.shape) != (G,) or not count.is_contiguous():
        raise KvqError(f"latent_group_sum: count must be a contiguous int64 [{G}]")
    if group.dtype != torch.int32 or tuple(group.shape) != (B,) or not group.is_contiguous():
        raise KvqError(f"latent_group_sum: group must be a contiguous int32 [{B}], got {group.dtype} {tuple(group.shape)}")
    if n_bad is not None and (n_bad.dtype != torch.int32 or n_bad.numel() != 1):
        raise KvqError("latent_group_sum: n_bad must be one int32 word")
    l = lib()
    nws = l.kvq_latent_group_sum_workspace_bytes(B, S, H, G)
    ws = _workspace(x.device, nws)               # slabs: written and consumed inside this call, on this stream
    check(l.kvq_latent_group_sum(x.data_ptr(), ldx, group.data_ptr(), B, S, H, G, io_dtype_of(x), table.data_ptr(), count.data_ptr(),
                                 _p(n_bad), ws.data_ptr(), nws, stream_ptr()), "kvq_latent_group_sum")


def latent_shift(x, table, count, g1, g0, alpha=1.0, sel=None, out=None):
    """out = x + alpha * (table[g1] / count[g1] - table[g0] / count[g0]) at the positions with sel[b, s] != 0 (sel [B, S] int8, None
    = all), x elsewhere (kvq_latent_shift: f64 arithmetic -> f32 -> the dtype of x).  out: None = a new tensor, or x itself."""
    require_gpu(x, table, count, sel, out)
    B, S, H, ldx = _rows3(x, "latent_shift")
    G = table.shape[0] if table.dim() == 3 else -1
    if table.dtype != torch.float64 or tuple(table.shape) != (G, S, H) or not table.is_contiguous():
        raise KvqError(f"latent_shift: table must be a contiguous float64 [G, {S}, {H}], got {table.dtype} {tuple(table.shape)}")
    if count.dtype != torch.int64 or tuple(count.shape) != (G,) or not count.is_contiguous():
        raise KvqError(f"latent_shift: count must be a contiguous int64 [{G}]")
    if not (0 <= int(g1) < G and 0 <= int(g0) < G):
        raise KvqError(f"latent_shift: groups {g1}, {g0} outside [0, {G})")
    if sel is not None and (sel.dtype != torch.int8 or tuple(sel.shape) != (B, S) or not sel.is_contiguous()):
        raise KvqError(f"latent_shift: sel must be a contiguous int8 [{B}, {S}], got {sel.dtype} {tuple(sel.shape)}")
    if out is None:
        out = torch.empty((B, S, H), dtype=x.dtype, device=x.device)
    if out.dtype != x.dtype or tuple(out.shape) != (B, S, H):
        raise KvqError("latent_shift: out must have the shape and dtype of x")
    ldo = _rows3(out, "latent_shift (out)")[3]
    check(lib().kvq_latent_shift(x.data_ptr(), ldx, table.data_ptr(), count.data_ptr(), int(g1), int(g0), float(alpha), _p(sel), B, S, H, G,
                                 io_dtype_of(x), out.data_ptr(), ldo, stream_ptr()), "kvq_latent_shift")
    return out


def vq_lookup(indices, codebook, n_codes, dtype, out=None, n_bad=None):
    """out [N, G * Dg] (dtype f32 / bf16) = the codebook rows of indices [N, G] int64: out[n, g*Dg:(g+1)*Dg] = codebook[g*K + idx[n, g]]
    for the f32 codebook [G * K, Dg] (the `embedding.weight` layout of VectorQuantizer / MultiVectorQuantizer) -- kvq_vq_lookup.
    An index outside [0, K) leaves a zero row and is counted in n_bad ([1] int32, optional)."""
    require_gpu(indices, codebook, out, n_bad)
    if indices.dtype != torch.int64 or indices.dim() != 2 or not indices.is_contiguous():
        raise KvqError(f"vq_lookup: indices must be a contiguous int64 [N, G], got {indices.dtype} {tuple(indices.shape)}")
    N, G = indices.shape
    K = int(n_codes)
    if codebook.dtype != torch.float32 or codebook.dim() != 2 or codebook.shape[0] != G * K or not codebook.is_contiguous():
        raise KvqError(f"vq_lookup: the codebook must be a contiguous float32 [{G} * {K}, Dg], got {codebook.dtype} {tuple(codebook.shape)}")
    Dg = codebook.shape[1]
    if out is None:
        out = torch.empty((N, G * Dg), dtype=dtype, device=indices.device)
    if out.dtype != dtype or tuple(out.shape) != (N, G * Dg) or out.stride(1) != 1:
        raise KvqError(f"vq_lookup: out must be {dtype} [{N}, {G * Dg}] with unit column stride")
    if n_bad is not None and (n_bad.dtype != torch.int32 or n_bad.numel() != 1):
        raise KvqError("vq_lookup: n_bad must be one int32 word")
    check(lib().kvq_vq_lookup(indices.data_ptr(), codebook.data_ptr(), N, K, Dg, G, io_dtype_of(out), out.data_ptr(),
                              out.stride(0) if N > 1 else max(out.stride(0), G * Dg), _p(n_bad), stream_ptr()), "kvq_vq_lookup")
    return out


def attn_fwd_fp8_ok(Sq, Sk):
    return bool(lib().kvq_attn_fwd_fp8_ok(int(Sq), int(Sk)))


def attn_fwd_fp8(q, k, v, mask, B, nh, Sq, Sk, causal, p_drop, seed, site, state):
    """attn_fwd plus the fp8 copy of the context for the fp8 BertSelfOutput.dense: (ctx, lse, ctx8) -- see ln_fwd_fp8."""
    require_gpu(q, k, v)
    dh = 64
    assert q.dtype == torch.bfloat16
    ctx = torch.empty((B * Sq, nh * dh), dtype=q.dtype, device=q.device)
    ctx8 = torch.empty((B * Sq, nh * dh), dtype=torch.uint8, device=q.device)
    lse = torch.empty((B, nh, Sq), dtype=torch.float32, device=q.device)
    check(lib().kvq_attn_fwd_fp8(q.data_ptr(), k.data_ptr(), v.data_ptr(), _p(mask), B, nh, Sq, Sk, dh, q.stride(0), k.stride(0),
                                 v.stride(0), ctx.stride(0), int(causal), 1.0 / 8.0, float(p_drop), int(seed), int(site),
                                 ctx.data_ptr(), lse.data_ptr(), ctx8.data_ptr(), ctx8.stride(0), state.data_ptr(), stream_ptr()),
          "kvq_attn_fwd_fp8")
    return ctx, lse, ctx8


def attn_bwd(q, k, v, mask, g_ctx, B, nh, Sq, Sk, causal, p_drop, seed, site, g_q, g_k, g_v, bias_part_q=None, bias_part_k=None,
             bias_part_v=None, ctx=None, lse=None):
    """Writes g_q / g_k / g_v (same layouts / row strides as q / k / v).  bias_part_* (f32 2-D views with B rows, row stride
    free, k and v sharing one) receive the per-batch column sums of g_q / g_k / g_v = partial rows of the projection-bias gradients."""
    dh = 64
    assert g_q.stride(0) == q.stride(0) and g_k.stride(0) == k.stride(0) and g_v.stride(0) == v.stride(0)
    ldp_q = bias_part_q.stride(0) if bias_part_q is not None else 0
    kv_ref = bias_part_k if bias_part_k is not None else bias_part_v
    ldp_kv = kv_ref.stride(0) if kv_ref is not None else 0
    for t in (bias_part_q, bias_part_k, bias_part_v):
        assert t is None or (t.dtype == torch.float32 and t.shape[0] == B and t.shape[1] >= nh * dh and t.stride(1) == 1)
    assert bias_part_k is None or bias_part_v is None or bias_part_k.stride(0) == bias_part_v.stride(0)
    if ctx is not None and lse is not None:       # the forward's output and log-sum-exp: what the kernels above 32 tokens work from
        assert ctx.stride(0) == g_ctx.stride(0) and lse.is_contiguous() and lse.dtype == torch.float32
        check(lib().kvq_attn_bwd_saved(q.data_ptr(), k.data_ptr(), v.data_ptr(), _p(mask), ctx.data_ptr(), lse.data_ptr(), g_ctx.data_ptr(),
                                       B, nh, Sq, Sk, dh, q.stride(0), k.stride(0), v.stride(0), g_ctx.stride(0), int(causal), 1.0 / 8.0,
                                       float(p_drop), int(seed), int(site), io_dtype_of(q), g_q.data_ptr(), g_k.data_ptr(), g_v.data_ptr(),
                                       _p(bias_part_q), _p(bias_part_k), _p(bias_part_v), int(ldp_q), int(ldp_kv), stream_ptr()),
              "kvq_attn_bwd_saved")
        return
    check(lib().kvq_attn_bwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), _p(mask), g_ctx.data_ptr(), B, nh, Sq, Sk, dh, q.stride(0),
                             k.stride(0), v.stride(0), g_ctx.stride(0), int(causal), 1.0 / 8.0, float(p_drop), int(seed), int(site),
                             io_dtype_of(q), g_q.data_ptr(), g_k.data_ptr(), g_v.data_ptr(), _p(bias_part_q), _p(bias_part_k),
                             _p(bias_part_v), int(ldp_q), int(ldp_kv), stream_ptr()), "kvq_attn_bwd")


def _adam_args(p32, g, m, v, vmax, shadow, step_state, beta1, beta2, eps, weight_decay, grad_scale):
    """What every kvq_adam_step* entry starts with (kvq_adam_step has lr where the others have the step state)."""
    return (p32.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), _p(vmax), _p(shadow), p32.numel(), io_dtype_of(g), _p(step_state),
            float(beta1), float(beta2), float(eps), float(weight_decay), float(grad_scale))


def _adam_call(name, guarded_name, args, guard):
    """One Adam entry, or with a gradient guard its guarded form, which takes the guard state last."""
    if guard is not None:
        name, args = guarded_name, args + (_guard_ptr(guard),)
    check(getattr(lib(), name)(*args, stream_ptr()), name)


def adam_step(p32, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, vmax=None, shadow=None, grad_scale=1.0):
    a = _adam_args(p32, g, m, v, vmax, shadow, None, beta1, beta2, eps, weight_decay, grad_scale)
    check(lib().kvq_adam_step(*a[:8], float(lr), *a[9:13], int(step), a[13], stream_ptr()), "kvq_adam_step")


def adam_step_dev(p32, g, m, v, step_state, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, vmax=None, shadow=None, grad_scale=1.0,
                  guard=None, fp8=None):
    """adam_step with lr and the bias corrections read on the device from `step_state` (see step_state_advance).  guard: a gradient
    guard state (new_grad_guard): the gradient is scaled by grad_scale * guard.coef, and nothing is stored when guard.skip is set.
    fp8: (mirror, span_segment, seg_scale, seg_off, seg_n, nseg, first_element) of kvq_adam_step_dev_fp8 (include/kvq.h): the update
    also writes the fp8 mirror of the GEMM weights among its elements."""
    args = _adam_args(p32, g, m, v, vmax, shadow, step_state, beta1, beta2, eps, weight_decay, grad_scale)
    if fp8 is None:
        return _adam_call("kvq_adam_step_dev", "kvq_adam_step_guarded", args, guard)
    *tables, nseg, first_element = fp8
    _adam_call("kvq_adam_step_dev_fp8", "kvq_adam_step_guarded_fp8",
               args + tuple(t.data_ptr() for t in tables) + (int(nseg), int(first_element)), guard)


def new_step_state(device):
    """24 zeroed bytes: struct { uint64 step; float lr, bc1, bc2s, pad; } of include/kvq.h."""
    return torch.zeros(3, dtype=torch.int64, device=device)


def _step_state_args(step_state, lr0, gamma, milestones, beta1, beta2):
    import ctypes
    ms = [int(x) for x in milestones]
    return (step_state.data_ptr(), float(lr0), float(gamma), (ctypes.c_int64 * max(len(ms), 1))(*ms), len(ms), float(beta1), float(beta2))


def step_state_advance(step_state, lr0, gamma, milestones, beta1, beta2):
    """step += 1 and the lr / bias corrections of that step."""
    check(lib().kvq_step_state_advance(*_step_state_args(step_state, lr0, gamma, milestones, beta1, beta2), stream_ptr()),
          "kvq_step_state_advance")


LR_DECAY_KINDS = {"none": 0, "linear": 1, "cosine": 2}       # decay_kind of kvq_step_state_advance_sched


def step_state_advance_sched(step_state, lr0, gamma, milestones, beta1, beta2, warmup_steps=0, decay_kind=0, total_steps=0, min_ratio=0.0):
    """step_state_advance with a linear warm-up over `warmup_steps` steps and a linear (1) / cosine (2) decay to min_ratio * lr0 at
    `total_steps` (include/kvq.h); warmup_steps 0 and decay_kind 0 give step_state_advance's bits."""
    check(lib().kvq_step_state_advance_sched(*_step_state_args(step_state, lr0, gamma, milestones, beta1, beta2), int(warmup_steps),
                                             int(decay_kind), int(total_steps), float(min_ratio), stream_ptr()),
          "kvq_step_state_advance_sched")


def adam_step_grouped(p32, g, m, v, step_state, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, vmax=None, shadow=None, grad_scale=1.0,
                      guard=None, block_group=None, first_element=0, group_lr_scale=None, group_wd=None, n_groups=1, decoupled=False):
    """adam_step_dev with parameter groups (include/kvq.h): block_group (uint8, one entry per 16-element block of the flat buffer the
    range was cut from; p32[0] is element first_element of that buffer) names each block's entry of the f32 device tables
    group_lr_scale / group_wd (None: scale 1 / weight_decay for every group).  block_group None: entry 0 for the whole launch.
    decoupled: torch.optim.AdamW's decay instead of the coupled L2 term."""
    n = p32.numel()
    for t, dt in ((block_group, torch.uint8), (group_lr_scale, torch.float32), (group_wd, torch.float32)):
        if t is not None and (t.dtype != dt or not t.is_cuda or not t.is_contiguous()):
            raise KvqError(f"adam_step_grouped: the group tables are contiguous device tensors (uint8 blocks, f32 scales and decays)")
    if block_group is not None and (first_element % 16 or (first_element + n + 15) // 16 > block_group.numel()):
        raise KvqError(f"adam_step_grouped: elements [{first_element}, {first_element + n}) need a first element that is a multiple of 16 "
                       f"and {(first_element + n + 15) // 16} table blocks, the table has {block_group.numel()}")
    for t in (group_lr_scale, group_wd):
        if t is not None and t.numel() < n_groups:
            raise KvqError(f"adam_step_grouped: {n_groups} groups, a table of {t.numel()}")
    args = _adam_args(p32, g, m, v, vmax, shadow, step_state, beta1, beta2, eps, weight_decay, grad_scale)
    _adam_call("kvq_adam_step_grouped", "kvq_adam_step_grouped_guarded",
               args + (_p(block_group), int(first_element), _p(group_lr_scale), _p(group_wd), int(n_groups), int(bool(decoupled))), guard)


def read_step_state(step_state):
    """(step, lr, bc1, bc2s) -- synchronises; for tests and logging."""
    raw = step_state.cpu()
    f = raw[1:].view(torch.float32)
    return int(raw[0]), float(f[0]), float(f[1]), float(f[2])


# ---- gradient guard (include/kvq.h "gradient guard"): global gradient norm, clipping coefficient, non-finite step skip -----------
def grad_sumsq_partials():
    """Partial sums one grad_sumsq_partial call writes (a constant of the library)."""
    return int(lib().kvq_grad_sumsq_partials())


def new_grad_guard(device):
    """32 zeroed bytes: struct { double sumsq; float norm, coef; uint32 skip, pad; uint64 skipped; } of include/kvq.h."""
    return torch.zeros(4, dtype=torch.int64, device=device)


def _guard_ptr(guard):
    if not torch.is_tensor(guard) or guard.dtype != torch.int64 or guard.numel() != 4 or not guard.is_contiguous():
        raise KvqError("a gradient guard state is new_grad_guard()'s tensor (4 x int64)")
    require_gpu(guard)
    return guard.data_ptr()


def read_grad_guard(guard):
    """dict(norm, coef, skip, skipped, sumsq) -- synchronises; for tests, logging and TrainEngine.skipped_steps."""
    _guard_ptr(guard)
    raw = guard.cpu()
    f = raw[1:2].view(torch.float32)
    return dict(norm=float(f[0]), coef=float(f[1]), skip=int(raw[2]) & 0xFFFFFFFF, skipped=int(raw[3]),
                sumsq=float(raw[0:1].view(torch.float64)[0]))


def grad_sumsq_partial(g, partials):
    """partials (f64, grad_sumsq_partials() elements, e.g. a slice of a larger buffer) = partial sums of g**2 over the flat f32 / bf16
    tensor g.  Deterministic; see include/kvq.h."""
    require_gpu(g, partials)
    if not g.is_contiguous() or g.numel() < 1:
        raise KvqError("grad_sumsq_partial: a contiguous gradient of at least one element required")
    if partials.dtype != torch.float64 or not partials.is_contiguous():
        raise KvqError("grad_sumsq_partial: the partial sums are a contiguous float64 tensor")
    check(lib().kvq_grad_sumsq_partial(g.data_ptr(), g.numel(), io_dtype_of(g), partials.data_ptr(), partials.numel(), stream_ptr()),
          "kvq_grad_sumsq_partial")


def grad_guard_finalize(partials, max_norm, guard):
    """All partial sums of the step -> guard: norm, coef = min(1, max_norm / (norm + 1e-6)), or skip when the sum is not finite."""
    require_gpu(partials)
    if partials.dtype != torch.float64 or not partials.is_contiguous():
        raise KvqError("grad_guard_finalize: the partial sums are a contiguous float64 tensor")
    check(lib().kvq_grad_guard_finalize(partials.data_ptr(), partials.numel(), float(max_norm), _guard_ptr(guard), stream_ptr()),
          "kvq_grad_guard_finalize")


# ---- gradient accumulation (include/kvq.h "gradient accumulation"): f32 sum of the micro-batch gradients, mean on the last one ----
def new_accum_state(device):
    """16 zeroed bytes: struct { uint64 tick; uint32 micro, pad; } of include/kvq.h."""
    return torch.zeros(2, dtype=torch.int64, device=device)


def _accum_ptr(state):
    if not torch.is_tensor(state) or state.dtype != torch.int64 or state.numel() != 2 or not state.is_contiguous():
        raise KvqError("an accumulation state is new_accum_state()'s tensor (2 x int64)")
    require_gpu(state)
    return state.data_ptr()


def read_accum_state(state):
    """(tick, micro) -- synchronises; for tests and TrainEngine's bookkeeping checks."""
    _accum_ptr(state)
    raw = state.cpu()
    return int(raw[0]), int(raw[1]) & 0xFFFFFFFF


def grad_accumulate(g, acc, state, A):
    """acc (f32, as long as g) = g on the first micro-step of a cycle, acc + g on the others, (acc + g) * (1 / A) on the last;
    the position is read on the device from `state` (new_accum_state).  g: a flat contiguous f32 / bf16 tensor."""
    require_gpu(g, acc)
    if not g.is_contiguous() or g.numel() < 1:
        raise KvqError("grad_accumulate: a contiguous gradient of at least one element required")
    if acc.dtype != torch.float32 or not acc.is_contiguous() or acc.numel() != g.numel():
        raise KvqError("grad_accumulate: the accumulator is a contiguous float32 tensor of the gradient's length")
    check(lib().kvq_grad_accumulate(g.data_ptr(), g.numel(), io_dtype_of(g), acc.data_ptr(), _accum_ptr(state), int(A), stream_ptr()),
          "kvq_grad_accumulate")


def accum_advance(state, A):
    """tick += 1, micro = (micro + 1) mod A, on the device."""
    check(lib().kvq_accum_advance(_accum_ptr(state), int(A), stream_ptr()), "kvq_accum_advance")


# ---- free-running generation (include/kvq.h "free-running generation"; csrc/kvq_generate.hip) -------------------------------------
GEN_MAX_KEYS = 128


def new_gen_state(device, t=0, prompt_len=1, max_length=1, eos_id=None, pad_id=0, temperature=0.0, seed=0):
    """32 bytes: struct { int32 t, P, Lmax, eos_id, pad_id; uint32 seed_lo, seed_hi; float inv_tau; } of include/kvq.h.
    eos_id None = no end token (-1); temperature 0 = greedy (inv_tau 0)."""
    return torch.tensor(gen_state_words(t, prompt_len, max_length, eos_id, pad_id, temperature, seed), dtype=torch.int32).to(device)


def _i32(u):
    """the int32 with the bits of the uint32 u"""
    u &= 0xFFFFFFFF
    return u - (1 << 32) if u >= (1 << 31) else u


def gen_state_words(t, prompt_len, max_length, eos_id, pad_id, temperature=0.0, seed=0):
    """The eight int32 words of a generation state.  temperature > 0: the words carry the f32 bits of 1 / temperature and the
    64-bit Philox key; 0: greedy."""
    import struct
    if not (float(temperature) >= 0.0) or float(temperature) == float("inf"):
        raise KvqError(f"a generation state takes a finite temperature >= 0 (0 = greedy), got {temperature!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < (1 << 64):
        raise KvqError(f"a generation state takes a seed in [0, 2^64), got {seed!r}")
    inv = 1.0 / float(temperature) if temperature > 0 else 0.0
    if inv > 3.0e38:                         # (no f32 holds it)
        raise KvqError(f"a generation state cannot hold 1 / temperature for temperature {temperature!r}")
    bits = struct.unpack("<I", struct.pack("<f", inv))[0]
    return [int(t), int(prompt_len), int(max_length), -1 if eos_id is None else int(eos_id), int(pad_id), _i32(seed), _i32(seed >> 32),
            _i32(bits)]


def _gen_ptr(state):
    if not torch.is_tensor(state) or state.dtype != torch.int32 or state.numel() != 8 or not state.is_contiguous():
        raise KvqError("a generation state is new_gen_state()'s tensor (8 x int32)")
    require_gpu(state)
    return state.data_ptr()


def read_gen_state(state):
    """dict(t, P, Lmax, eos_id, pad_id, seed, inv_tau) -- synchronises; for tests."""
    import struct
    _gen_ptr(state)
    w = state.cpu().tolist()
    return dict(t=w[0], P=w[1], Lmax=w[2], eos_id=w[3], pad_id=w[4], seed=(w[5] & 0xFFFFFFFF) | ((w[6] & 0xFFFFFFFF) << 32),
                inv_tau=struct.unpack("<f", struct.pack("<I", w[7] & 0xFFFFFFFF))[0])


def gen_embed(state, ids, word, pos, type_row, gamma, beta, eps, out=None):
    """out [B, H] = LayerNorm(word[ids[b, t]] + pos[t] + type_row), t read from the state on the device: the bits of
    embed_ln_fwd's row for the same token at the same position (no dropout)."""
    require_gpu(ids, word, pos, type_row, gamma, beta)
    if ids.dim() != 2 or ids.dtype != torch.int64 or not ids.is_contiguous():
        raise KvqError("kvq.nnops.gen_embed: ids must be a contiguous int64 [B, Lmax] tensor")
    B, H = ids.shape[0], word.shape[1]
    if out is None:
        out = torch.empty((B, H), dtype=word.dtype, device=word.device)
    check(lib().kvq_gen_embed(_gen_ptr(state), ids.data_ptr(), word.data_ptr(), pos.data_ptr(), type_row.data_ptr(), gamma.data_ptr(),
                              beta.data_ptr(), B, H, word.shape[0], pos.shape[0], float(eps), io_dtype_of(word), out.data_ptr(), stream_ptr()),
          "kvq_gen_embed")
    return out


def _gen_rows(who, x, name):
    if x.dim() != 2 or x.stride(1) != 1:
        raise KvqError(f"kvq.nnops.{who}: {name} must be 2-D with unit column stride")
    return x.stride(0)


def gen_attn_self(state, q, k_new, v_new, cache, nh, out=None):
    """One query row per (sentence, head) against the cache [B, Smax, 2 nh 64]: this step's k_new | v_new rows (column slices of the
    fused projection, [B, nh 64] each, one row stride) are stored to row t first, then rows 0 .. t are attended.  t: from the state."""
    require_gpu(q, k_new, v_new, cache)
    B, W = q.shape[0], nh * 64
    ldq, ldn = _gen_rows("gen_attn_self", q, "q"), _gen_rows("gen_attn_self", k_new, "k_new")
    if _gen_rows("gen_attn_self", v_new, "v_new") != ldn or k_new.shape != (B, W) or v_new.shape != (B, W) or q.shape[1] != W:
        raise KvqError(f"kvq.nnops.gen_attn_self: q, k_new, v_new must be [B, {W}] and k_new, v_new share a row stride")
    if cache.dim() != 3 or cache.shape[0] != B or cache.shape[2] != 2 * W or not cache.is_contiguous() or cache.dtype != q.dtype:
        raise KvqError(f"kvq.nnops.gen_attn_self: the cache must be a contiguous [B, Smax, {2 * W}] tensor of q's dtype")
    if out is None:
        out = torch.empty((B, W), dtype=q.dtype, device=q.device)
    check(lib().kvq_gen_attn(_gen_ptr(state), q.data_ptr(), ldq, k_new.data_ptr(), v_new.data_ptr(), ldn, cache.data_ptr(), cache.stride(1),
                             cache.stride(0), B, nh, 1, 0, cache.shape[1], io_dtype_of(q), out.data_ptr(), _gen_rows("gen_attn_self", out, "out"),
                             stream_ptr()), "kvq_gen_attn")
    return out


def gen_attn_cross(state, q, kv, n_keys, nh, out=None):
    """The same against n_keys given rows per sentence: kv [B * n_keys, >= 2 nh 64] = keys | values (a column slice of the all-layer
    projection of the latent is fine: its row stride is used).  No mask."""
    require_gpu(q, kv)
    B, W = q.shape[0], nh * 64
    ldq, ldk = _gen_rows("gen_attn_cross", q, "q"), _gen_rows("gen_attn_cross", kv, "kv")
    if q.shape[1] != W or kv.shape[0] != B * n_keys or kv.shape[1] != 2 * W or kv.dtype != q.dtype:
        raise KvqError(f"kvq.nnops.gen_attn_cross: q [B, {W}] needs kv [B * n_keys, {2 * W}] of its dtype, got {tuple(kv.shape)}")
    if out is None:
        out = torch.empty((B, W), dtype=q.dtype, device=q.device)
    check(lib().kvq_gen_attn(_gen_ptr(state), q.data_ptr(), ldq, None, None, 0, kv.data_ptr(), ldk, int(n_keys) * ldk, B, nh, 0, int(n_keys), 0,
                             io_dtype_of(q), out.data_ptr(), _gen_rows("gen_attn_cross", out, "out"), stream_ptr()), "kvq_gen_attn")
    return out


def gen_select(state, logits, V, ids, finished, lengths, step_logits=None):
    """The next token of every sentence: ids[b, t + 1] = first arg-max over v < V of logits[b, v] (the state's temperature 0) or a
    draw from softmax(logits / temperature) by the Gumbel-max trick (Philox keyed by the state's seed, t, b, v); prompt tokens are
    kept, a finished sentence gets the pad id, the end token finishes one (include/kvq.h).  Temperature and seed live in the
    state (new_gen_state), as t does.  step_logits [B, Lmax, V] f32: row (b, t) = the logits."""
    require_gpu(logits, ids, finished, lengths)
    B = logits.shape[0]
    ld = _gen_rows("gen_select", logits, "logits")
    if ids.dim() != 2 or ids.dtype != torch.int64 or not ids.is_contiguous() or ids.shape[0] != B:
        raise KvqError("kvq.nnops.gen_select: ids must be a contiguous int64 [B, Lmax] tensor")
    for name, x in (("finished", finished), ("lengths", lengths)):
        if x.dtype != torch.int32 or x.shape != (B,) or not x.is_contiguous():
            raise KvqError(f"kvq.nnops.gen_select: {name} must be a contiguous int32 [B] tensor")
    if step_logits is not None and (step_logits.dtype != torch.float32 or tuple(step_logits.shape) != (B, ids.shape[1], V)
                                    or not step_logits.is_contiguous()):
        raise KvqError(f"kvq.nnops.gen_select: step_logits must be a contiguous float32 [B, Lmax, V] = {(B, ids.shape[1], V)} tensor")
    check(lib().kvq_gen_select(_gen_ptr(state), logits.data_ptr(), ld, int(V), B, io_dtype_of(logits), ids.data_ptr(), finished.data_ptr(),
                               lengths.data_ptr(), _p(step_logits), stream_ptr()), "kvq_gen_select")


GEN_FILTER_MAX_V = 32768      # the columns kvq_gen_select_filtered holds in registers (csrc/kvq_generate.hip FLT_MAX_V)


def gen_filter_words(top_k=0, top_p=1.0):
    """The four int32 words of a filter state: struct { int32 top_k; float top_p; int32 reserved[2]; } of include/kvq.h.
    top_k 0 = off, top_p 1 = off."""
    import struct
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 0 <= top_k < (1 << 31):
        raise KvqError(f"a filter state takes top_k as an int >= 0 (0 = off), got {top_k!r}")
    if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not 0.0 < float(top_p) <= 1.0:
        raise KvqError(f"a filter state takes a finite top_p in (0, 1] (1 = off), got {top_p!r}")
    return [int(top_k), _i32(struct.unpack("<I", struct.pack("<f", float(top_p)))[0]), 0, 0]


def new_gen_filter(device, top_k=0, top_p=1.0):
    """16 bytes beside the generation state: what kvq_gen_select_filtered keeps (gen_filter_words)."""
    return torch.tensor(gen_filter_words(top_k, top_p), dtype=torch.int32).to(device)


def _filter_ptr(filt):
    if not torch.is_tensor(filt) or filt.dtype != torch.int32 or filt.numel() != 4 or not filt.is_contiguous():
        raise KvqError("a filter state is new_gen_filter()'s tensor (4 x int32)")
    require_gpu(filt)
    return filt.data_ptr()


def gen_select_filtered(state, filt, logits, V, ids, finished, lengths, step_logits=None, step_kept=None, step_cut=None, step_logprob=None):
    """gen_select on the distribution the filter state `filt` (new_gen_filter) leaves: the first top_k of the order (logit
    descending, then index ascending), of those the shortest prefix whose mass reaches top_p; the same noise, so with the filters
    off the bits of gen_select.  step_kept / step_cut int32, step_logprob f32, [B, Lmax] each: row (b, t) = the size of the kept
    set, the id of its last element, the log-probability of the choice under the distribution sampled from (include/kvq.h)."""
    require_gpu(logits, ids, finished, lengths)
    B = logits.shape[0]
    ld = _gen_rows("gen_select_filtered", logits, "logits")
    if isinstance(V, bool) or not isinstance(V, int) or not 1 <= V <= GEN_FILTER_MAX_V:
        raise KvqError(f"kvq.nnops.gen_select_filtered: V must be an int in 1 .. {GEN_FILTER_MAX_V} (the columns a workgroup holds), got {V!r}")
    if ids.dim() != 2 or ids.dtype != torch.int64 or not ids.is_contiguous() or ids.shape[0] != B:
        raise KvqError("kvq.nnops.gen_select_filtered: ids must be a contiguous int64 [B, Lmax] tensor")
    for name, x in (("finished", finished), ("lengths", lengths)):
        if x.dtype != torch.int32 or x.shape != (B,) or not x.is_contiguous():
            raise KvqError(f"kvq.nnops.gen_select_filtered: {name} must be a contiguous int32 [B] tensor")
    if step_logits is not None and (step_logits.dtype != torch.float32 or tuple(step_logits.shape) != (B, ids.shape[1], V)
                                    or not step_logits.is_contiguous()):
        raise KvqError(f"kvq.nnops.gen_select_filtered: step_logits must be a contiguous float32 [B, Lmax, V] = {(B, ids.shape[1], V)} tensor")
    for name, x, dt in (("step_kept", step_kept, torch.int32), ("step_cut", step_cut, torch.int32), ("step_logprob", step_logprob, torch.float32)):
        if x is not None and (x.dtype != dt or tuple(x.shape) != tuple(ids.shape) or not x.is_contiguous()):
            raise KvqError(f"kvq.nnops.gen_select_filtered: {name} must be a contiguous {dt} [B, Lmax] = {tuple(ids.shape)} tensor")
    check(lib().kvq_gen_select_filtered(_gen_ptr(state), _filter_ptr(filt), logits.data_ptr(), ld, V, B, io_dtype_of(logits), ids.data_ptr(),
                                        finished.data_ptr(), lengths.data_ptr(), _p(step_logits), _p(step_kept), _p(step_cut), _p(step_logprob),
                                        stream_ptr()), "kvq_gen_select_filtered")


def gen_gumbel_debug(bits):
    """g [n] f32 = the Gumbel(0, 1) value kvq_gen_select forms from each of the 32-bit patterns bits [n] (int64 holding 0 .. 2^32 - 1,
    or int32 holding the bits): a test hook."""
    require_gpu(bits)
    if bits.dtype == torch.int64:
        bits = (bits & 0xFFFFFFFF).to(torch.int32)      # (the low 32 bits, two's complement)
    if bits.dtype != torch.int32 or bits.dim() != 1 or not bits.is_contiguous() or bits.numel() < 1:
        raise KvqError("kvq.nnops.gen_gumbel_debug: a contiguous 1-D int32 / int64 tensor of bit patterns required")
    out = torch.empty(bits.numel(), dtype=torch.float32, device=bits.device)
    check(lib().kvq_gen_gumbel_debug(bits.data_ptr(), bits.numel(), out.data_ptr(), stream_ptr()), "kvq_gen_gumbel_debug")
    return out


def gen_advance(state):
    """t += 1, on the device."""
    check(lib().kvq_gen_advance(_gen_ptr(state), stream_ptr()), "kvq_gen_advance")


# ---- EMA of the trained weights (include/kvq.h "exponential moving average of the trained weights") -------------------------------
def new_weight_ema_state(device):
    """16 zeroed bytes: struct { uint64 updates; float last_decay; uint32 pad; } of include/kvq.h."""
    return torch.zeros(2, dtype=torch.int64, device=device)


def _wema_ptr(state):
    if not torch.is_tensor(state) or state.dtype != torch.int64 or state.numel() != 2 or not state.is_contiguous():
        raise KvqError("a weight-EMA state is new_weight_ema_state()'s tensor (2 x int64)")
    require_gpu(state)
    return state.data_ptr()


def read_weight_ema_state(state):
    """(updates, last_decay) -- synchronises; for tests, logging and TrainEngine.weight_ema_updates."""
    _wema_ptr(state)
    raw = state.cpu()
    return int(raw[0]), float(raw[1:2].view(torch.float32)[0])


def _wema_pair(what, p, ema):
    require_gpu(p, ema)
    if p.dtype != torch.float32 or not p.is_contiguous() or p.numel() < 1:
        raise KvqError(f"{what}: contiguous float32 parameters of at least one element required")
    if ema.dtype != torch.float32 or not ema.is_contiguous() or ema.numel() != p.numel():
        raise KvqError(f"{what}: the average is a contiguous float32 tensor of the parameters' length")


def weight_ema_update(p, ema, state, decay, guard=None):
    """ema (f32, as long as p) = p on the first update, d * ema + (1 - d) * p in f64 on the others, d = min(decay, (1 + t) / (10 + t))
    with the update count t read on the device from `state` (new_weight_ema_state).  guard: a gradient guard state -- nothing is
    stored when guard.skip is set."""
    _wema_pair("weight_ema_update", p, ema)
    check(lib().kvq_weight_ema_update(p.data_ptr(), ema.data_ptr(), p.numel(), float(decay), _wema_ptr(state),
                                      _guard_ptr(guard) if guard is not None else None, stream_ptr()), "kvq_weight_ema_update")


def weight_ema_advance(state, decay, guard=None):
    """last_decay = the d of this step's updates (0 for the storing one), updates += 1, on the device; nothing when guard.skip is set."""
    check(lib().kvq_weight_ema_advance(_wema_ptr(state), float(decay), _guard_ptr(guard) if guard is not None else None, stream_ptr()),
          "kvq_weight_ema_advance")


def weight_ema_swap(p, ema, shadow=None):
    """p <-> ema, exactly; shadow (bf16, as long as p): the bf16 copy of the new p, rounded as the Adam kernel rounds its shadow."""
    _wema_pair("weight_ema_swap", p, ema)
    if shadow is not None:
        require_gpu(shadow)
        if shadow.dtype != torch.bfloat16 or not shadow.is_contiguous() or shadow.numel() != p.numel():
            raise KvqError("weight_ema_swap: the shadow is a contiguous bfloat16 tensor of the parameters' length")
    check(lib().kvq_weight_ema_swap(p.data_ptr(), ema.data_ptr(), _p(shadow), p.numel(), stream_ptr()), "kvq_weight_ema_swap")


def set_seed_offset(step_state):
    """Dropout-bearing kernels launched from now on use seed + step_state.step (read on the device); None switches it off.  (Any
    device tensor whose first word is a uint64 count will do: an accumulating engine passes its accumulation state.)"""
    check(lib().kvq_set_seed_offset(step_state.data_ptr() if step_state is not None else None), "kvq_set_seed_offset")


def dropout(x, p_drop, seed, site, out=None):
    """x * keep / (1 - p) with the Philox mask of (seed, site); applying it to a gradient is the backward."""
    require_gpu(x)
    xc = x.contiguous()
    o = torch.empty_like(xc) if out is None else out
    check(lib().kvq_dropout(xc.data_ptr(), xc.numel(), float(p_drop), int(seed), int(site), io_dtype_of(xc), o.data_ptr(), stream_ptr()),
          "kvq_dropout")
    return o


def zero_ranges(tensors):
    """Zero up to four contiguous tensors (16-byte aligned, sizes multiples of 16 bytes) in one launch."""
    import ctypes
    ts = [t for t in tensors if t is not None]
    if not ts:
        return
    ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    sizes = (ctypes.c_int64 * len(ts))(*[t.numel() * t.element_size() for t in ts])
    check(lib().kvq_zero_ranges(ptrs, sizes, len(ts), stream_ptr()), "kvq_zero_ranges")


def embed_grad(g, perm, sorted_ids, gW, accumulate=False):
    """gW[id] (= | +=) sum of g[n] over the tokens with that id, in token order (deterministic, no atomics).
    perm / sorted_ids: stable sort of the flattened ids (sorted_ids, perm = torch.sort(ids.reshape(-1), stable=True))."""
    require_gpu(g, gW)
    N, H = g.shape
    l = lib()
    ws = _workspace(g.device, l.kvq_embed_grad_workspace_bytes(N, H), tag="embed_grad")
    check(l.kvq_embed_grad(g.data_ptr(), perm.data_ptr(), sorted_ids.data_ptr(), N, H, gW.shape[0], io_dtype_of(g), gW.data_ptr(),
                           io_dtype_of(gW), int(accumulate), ws.data_ptr(), ws.numel(), stream_ptr()), "kvq_embed_grad")
    return gW


# ---- the GEMM family of csrc/kvq_gemm2.hip ---------------------------------------------------------------------------------
_LAYOUTS = {"nt": 0, "nn": 1, "tn": 2}
# "128x192h" (round 5): four waves, two ring slots, TWO workgroups per CU.  Faster than the persistent / 256 x 192 kernels on hot
# operands ([8192, 2304] x 768: 34.5 against 37.0 us; [8192, 3072]: 39.6 against 41.6) and slower inside the step, where the operands
# are cold and one k-tile of prefetch is not enough (QKV 35.6 against 31.9 us): kept as an explicit choice, not in pick_tile's set
# (profiles/r05_gemm_ceiling.md)
TILES = {"128x192": 0, "128x256": 1, "256x192": 2, "256x256": 3, "64x128": 4, "128x192h": 5,
         "128x192p": 0x100, "128x256p": 0x101, "256x192p": 0x102, "256x256p": 0x103}      # p: KVQ_GEMM_PERSISTENT (layout nt only)
TILE_NAMES = {v: k for k, v in TILES.items()}
_TILE_DIMS = {0: (128, 192), 1: (128, 256), 2: (256, 192), 3: (256, 256), 4: (64, 128)}
def _gemm_dims(a, b, layout):
    if layout == "nt":
        (M, K), N = a.shape, b.shape[0]
    elif layout == "nn":
        (M, K), N = a.shape, b.shape[1]
    else:
        (K, M), N = a.shape, b.shape[1]
    return M, N, K


# Cost model of one launch, microseconds, fitted to tools/gemm2_probe_small.py on MI355X (profiles/r04_gemm_small.md: 72 products at
# 768 .. 6144 rows x 5 tiles; mean regret of the model's pick against the best measured tile 0.7 %, worst 17 %) and consistent with
# the choices measured at 8192 rows in rounds 2 - 3 (tools/gemm2_probe.py):
#   per 64-deep k-tile of ONE workgroup: _TK_ALONE when few CUs are busy (operands come from L2 unopposed), _TK_FULL when all 256
#   are (the L2 -> LDS fill is shared); linear in the busy fraction between.  _T_TILE: start-up + epilogue of a tile.
#   The 64 x 128 tile (4 waves, 72 KiB of LDS) runs two workgroups per CU, which together take _TK_PAIR per k-tile.
_TK_ALONE = {0: 0.459, 1: 0.557, 2: 0.891, 3: 1.035, 4: 0.296}
_TK_FULL = {0: 0.825, 1: 0.98, 2: 1.5, 3: 1.83, 4: 0.40}
_TK_PAIR = (0.45, 0.52)
_T_TILE = {0: 1.5, 1: 2.0, 2: 2.5, 3: 3.0, 4: 1.0}


def tile_cost_us(t, M, N, K, n_cu=256):
    """Modelled duration of an [M, N] x K product on tile t (see the table above)."""
    bm, bn = _TILE_DIMS[t]
    n = -(-M // bm) * -(-N // bn)
    kt = max(K // 64, 1)
    f = min(n, n_cu) / n_cu
    lerp = lambda a, b: a + (b - a) * f
    w = -(-n // n_cu)                                    # workgroups the busiest CU runs
    if t == 4:
        return kt * ((w // 2) * lerp(*_TK_PAIR) + (w % 2) * lerp(_TK_ALONE[t], _TK_FULL[t])) + w * _T_TILE[t]
    return w * (kt * lerp(_TK_ALONE[t], _TK_FULL[t]) + _T_TILE[t])


def pick_tile(M, N, K=768, n_cu=256, candidates=None):
    """Workgroup tile for an [M, N] x K product: the cheapest under tile_cost_us() -- the rule over (M, N, K) that replaced the
    engine's exact-shape tables.  candidates: restrict the choice (the fused-activation epilogues exist for two tiles)."""
    cand = list(_TILE_DIMS) if candidates is None else [TILES[c] if isinstance(c, str) else c for c in candidates]
    return min(cand, key=lambda t: (tile_cost_us(t, M, N, K, n_cu), -_TILE_DIMS[t][0] * _TILE_DIMS[t][1]))


def persistent_pays(t, M, N, K, layout, accumulate=False, n_cu=256):
    """The persistent tile loop (KVQ_GEMM_PERSISTENT: NT only, whole tiles, no accumulate) instead of one tile per workgroup:
    when a CU owns 3 .. 12 tiles.  Measured at 8192 rows (tools/gemm2_probe_persist.py, profiles/NOTES_r01-r03_design_and_experiments.md section 2.3): QKV (3 tiles per CU)
    and the all-layer cross-K/V projection (9) gain 1 - 4 %, two tiles per CU (FFN1) lose, the LM head (15, column bands) loses 6 %."""
    bm, bn = _TILE_DIMS[t]
    if layout != "nt" or accumulate or t == 4 or M < bm or N < bn or K // 64 < 3:
        return False
    per_cu = -(-(-(-M // bm) * -(-N // bn)) // n_cu)
    return 3 <= per_cu <= 12


def cu_count(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


def mixed_split(M, N, n_cu):
    """The row split of the "mixed" tile of an [M, N] weight gradient: r rows -- the most whole 256-row tile rows that fit n_cu CUs
    once -- on 256 x 256 tiles and the other M - r on 128 x 256 tiles, when those fit the CUs once as well: one full round of the large
    tile and a shorter one of the small tile instead of up to three of the small one.  0: the shape does not split that way."""
    tn = -(-N // 256)
    r = n_cu // tn * 256
    return r if 0 < r < M and -(-(M - r) // 128) * tn <= n_cu else 0


def gemm_mfma_ok(a, b, out, layout, bias=None):
    """True when kvq_gemm_bf16 (LDS-DMA + MFMA, csrc/kvq_gemm2.hip) takes this product: K % 64 == 0; M, N and the leading dimensions
    in multiples of 8; 16-byte aligned operands (bias: 8); unit column stride."""
    M, N, K = _gemm_dims(a, b, layout)
    ts = [a, b] + ([out] if out is not None else [])
    return K % 64 == 0 and M % 8 == 0 and N % 8 == 0 and M >= 8 and N >= 8 \
        and all(t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0 for t in ts) \
        and (bias is None or (bias.data_ptr() % 8 == 0 and bias.stride(0) == 1))


def gemm_problem(a, b, out, layout, bias=None, accumulate=False):
    from ._ffi import GemmProblem
    M, N, K = _gemm_dims(a, b, layout)
    assert a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and out.dtype == torch.bfloat16
    assert a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1 and tuple(out.shape) == (M, N)
    return GemmProblem(a.data_ptr(), b.data_ptr(), out.data_ptr(), _p(bias), M, N, K, a.stride(0), b.stride(0), out.stride(0),
                       int(accumulate))


def pad_rows(t, rows_padded):
    """[rows_padded, cols] copy of a row-major 2-D tensor (unit column stride) with zero rows behind its own -- one kernel."""
    rows, cols = t.shape
    es = t.element_size()
    out = torch.empty((rows_padded, cols), dtype=t.dtype, device=t.device)
    check(lib().kvq_pad_rows(t.data_ptr(), rows, cols * es, t.stride(0) * es, out.data_ptr(), rows_padded, stream_ptr()), "kvq_pad_rows")
    return out


def _pad_ok(t):
    return t.dim() == 2 and t.stride(1) == 1 and (t.shape[1] * t.element_size()) % 16 == 0 and (t.stride(0) * t.element_size()) % 16 == 0 \
        and t.data_ptr() % 16 == 0


def tn_operands_k64(a, b):
    """The operands of a "tn" product (both [K, .], K = tokens) with K padded to the MFMA kernel's 64-deep k-tile by zero rows
    (which add nothing to a^T . b), or None when K % 64 == 0 already / the rows cannot be copied in 16-byte pieces.  A batch of
    100 sentences x 12 tokens (the last batch of an epoch, any odd batch size) would otherwise put every weight gradient of the
    step -- the [30528, 768] LM head included -- on the any-shape kernel."""
    K = a.shape[0]
    if K % 64 == 0 or not (_pad_ok(a) and _pad_ok(b)):
        return None
    Kp = (K + 63) // 64 * 64
    return pad_rows(a, Kp), pad_rows(b, Kp)


_ANY_WARNED = set()
GEMM_ROUTES = {"mfma": 0, "any": 0, "tn_padded": 0, "row_split": 0}      # launches of gemm() by route (tests read it)


def _warn_any(M, N, K, layout):
    """Once per shape: a product of more than 64 MFLOP that no MFMA route takes (the any-shape kernel is a scalar-FMA kernel)."""
    if 2.0 * M * N * K > 64e6 and (M, N, K, layout) not in _ANY_WARNED:
        _ANY_WARNED.add((M, N, K, layout))
        import warnings
        warnings.warn(f"kvq.nnops.gemm: {layout} product M={M} N={N} K={K} ({2e-6 * M * N * K:.0f} MFLOP) runs on the any-shape kernel: "
                      f"the MFMA kernel needs K % 64 == 0, M / N / leading dimensions % 8 == 0 and 16-byte aligned operands", stacklevel=3)


def _gemm_any(a, b, layout, bias, out, accumulate, warn=True):
    M, N, K = _gemm_dims(a, b, layout)
    if a.stride(1) != 1:
        a = a.contiguous()
    if b.stride(1) != 1:
        b = b.contiguous()
    if out.stride(1) != 1 or (bias is not None and bias.stride(0) != 1):
        raise KvqError("kvq.nnops.gemm: output rows / bias must be contiguous")
    if warn:
        _warn_any(M, N, K, layout)
    GEMM_ROUTES["any"] += 1
    check(lib().kvq_gemm_any_bf16(a.data_ptr(), b.data_ptr(), _p(bias), out.data_ptr(), M, N, K, a.stride(0), b.stride(0), out.stride(0),
                                  _LAYOUTS[layout], int(accumulate), stream_ptr()), "kvq_gemm_any_bf16")
    return out


def gemm(a, b, layout="nt", bias=None, out=None, accumulate=False, tile=None):
    """out[M,N] (= | +=) op(a) @ op(b) (+ bias), bf16 with f32 accumulation.  layout "nt": a[M,K], b[N,K];  "nn": a[M,K], b[K,N];
    "tn": a[K,M], b[K,N].  The MFMA GEMM of csrc/kvq_gemm2.hip whenever the product meets its requirements (gemm_mfma_ok), tile
    from pick_tile() unless given.  Products that miss them only through their TOKEN count still reach it: a "tn" contraction
    over tokens is zero-padded to a multiple of 64 (tn_operands_k64), an "nt" / "nn" product over a token count that is not a
    multiple of 8 runs its first M - M % 8 rows there and the last rows on the any-shape kernel of csrc/kvq_gemm_any.hip, which
    also takes everything else (with a warning above 64 MFLOP).  Never a vendor library.  tile "mixed" (plain "tn" products that
    mixed_split() splits): one launch on two tile shapes, see there."""
    require_gpu(a, b)
    M, N, K = _gemm_dims(a, b, layout)
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or (out is not None and out.dtype != torch.bfloat16):
        raise KvqError(f"kvq.nnops.gemm: bf16 operands only (got {a.dtype}, {b.dtype})")
    if out is None:
        out = torch.empty((M, N), dtype=a.dtype, device=a.device)
    if not gemm_mfma_ok(a, b, out, layout, bias):
        if layout == "tn" and K % 64 != 0 and K > 64:
            padded = tn_operands_k64(a, b)
            if padded is not None and gemm_mfma_ok(padded[0], padded[1], out, layout, bias):
                GEMM_ROUTES["tn_padded"] += 1
                return gemm(padded[0], padded[1], layout, bias=bias, out=out, accumulate=accumulate, tile=tile)
        if layout != "tn" and M % 8 != 0 and M > 8 and gemm_mfma_ok(a[:M - M % 8], b, out[:M - M % 8], layout, bias):
            M8 = M - M % 8
            GEMM_ROUTES["row_split"] += 1
            gemm(a[:M8], b, layout, bias=bias, out=out[:M8], accumulate=accumulate, tile=tile)
            _gemm_any(a[M8:], b, layout, bias, out[M8:], accumulate, warn=False)                 # (at most 7 rows)
            return out
        return _gemm_any(a, b, layout, bias, out, accumulate)
    if tile == "mixed":
        # one product on two tile shapes (kvq_gemm_grouped_mixed_bf16), split by rows from the CU count
        r = mixed_split(M, N, cu_count(a.device)) if layout == "tn" and bias is None and not accumulate else 0
        if not r:
            raise KvqError(f"kvq.nnops.gemm: tile 'mixed' is for plain tn products that mixed_split() splits (M={M} N={N} {layout})")
        from ._ffi import GemmProblem
        GEMM_ROUTES["mfma"] += 1
        parts = [GemmProblem(a_.data_ptr(), b.data_ptr(), o_.data_ptr(), None, o_.shape[0], N, K, a.stride(0), b.stride(0), out.stride(0), 0)
                 for a_, o_ in ((a[:, :r], out[:r]), (a[:, r:], out[r:]))]
        gemm_grouped_mixed(parts, ["256x256", "128x256"], "tn")
        return out
    if tile is None:
        t = pick_tile(M, N, K)
        if persistent_pays(t, M, N, K, layout, accumulate):
            t |= 0x100
    else:
        t = TILES[tile] if isinstance(tile, str) else tile
    GEMM_ROUTES["mfma"] += 1
    check(lib().kvq_gemm_bf16(a.data_ptr(), b.data_ptr(), _p(bias), out.data_ptr(), M, N, K, a.stride(0), b.stride(0), out.stride(0),
                              _LAYOUTS[layout], t, int(accumulate), stream_ptr()), "kvq_gemm_bf16")
    return out


def gemm_grouped(problems, layout, tile):
    """One launch over a list of gemm_problem()s of one layout (at most 16)."""
    from ._ffi import GemmProblem
    arr = (GemmProblem * len(problems))(*problems)
    t = TILES[tile] if isinstance(tile, str) else tile
    check(lib().kvq_gemm_grouped_bf16(arr, len(problems), _LAYOUTS[layout], t, stream_ptr()), "kvq_gemm_grouped_bf16")


def gemm_grouped_mixed(problems, tiles, layout="tn"):
    """One launch over a list of "tn" gemm_problem()s (at most 16), each on its own tile ("256x256" or "128x256"): the 256 x 256
    tiles run first.  Bit for bit what gemm_grouped() stores for each problem on its tile."""
    import ctypes
    from ._ffi import GemmProblem
    if len(tiles) != len(problems):
        raise KvqError("kvq.nnops.gemm_grouped_mixed: one tile per problem")
    arr = (GemmProblem * len(problems))(*problems)
    ts = (ctypes.c_int * len(tiles))(*[TILES[t] if isinstance(t, str) else t for t in tiles])
    check(lib().kvq_gemm_grouped_mixed_bf16(arr, ts, len(problems), _LAYOUTS[layout], stream_ptr()), "kvq_gemm_grouped_mixed_bf16")


def gemm_gelu(x, w, bias, tile="256x192"):
    """(h, gelu(h)) with h = x @ w.T + bias in one kernel (BertIntermediate, modeling_bert.py:325-337)."""
    M, K = x.shape
    N = w.shape[0]
    h = torch.empty((M, N), dtype=x.dtype, device=x.device)
    a = torch.empty_like(h)
    check(lib().kvq_gemm_bf16_gelu(x.data_ptr(), w.data_ptr(), _p(bias), h.data_ptr(), a.data_ptr(), M, N, K, x.stride(0), w.stride(0),
                                   h.stride(0), TILES[tile], stream_ptr()), "kvq_gemm_bf16_gelu")
    return h, a


DROPRES_TILES = ("128x192", "128x256", "64x128")


def gemm_dropres(x, w, bias, resid, p_drop, seed, site, tile=None):
    """pre = dropout(x @ w.T + bias, p_drop) + resid in one kernel: the LayerNorm input of BertSelfOutput / BertOutput
    (modeling_bert.py:282-296, 339-352), bit for bit what ln_fwd(x @ w.T + bias, resid, ..., p_drop, seed, site) stores as `pre`
    (same roundings, same Philox masks) -- so the block's forward is this + ln_fwd(pre, None, ..., p_drop=0) and its backward is
    unchanged.  The tile comes from pick_tile() over the tiles this epilogue is built for."""
    M, K = x.shape
    N = w.shape[0]
    assert tuple(resid.shape) == (M, N) and resid.dtype == torch.bfloat16 and resid.stride(1) == 1
    pre = torch.empty((M, N), dtype=x.dtype, device=x.device)
    assert resid.stride(0) == pre.stride(0)
    t = pick_tile(M, N, K, candidates=DROPRES_TILES) if tile is None else (TILES[tile] if isinstance(tile, str) else tile)
    GEMM_ROUTES["mfma"] += 1
    check(lib().kvq_gemm_bf16_dropres(x.data_ptr(), w.data_ptr(), _p(bias), resid.data_ptr(), pre.data_ptr(), M, N, K, x.stride(0),
                                      w.stride(0), pre.stride(0), t, float(p_drop), int(seed), int(site), stream_ptr()),
          "kvq_gemm_bf16_dropres")
    return pre


def gemm_dgelu(gy, w, h, tile="256x192"):
    """(g_h, part): g_h = (gy @ w) * gelu'(h) and part [rows, N] f32 partial column sums of g_h (bias-gradient partials for
    reduce_batch()) in one kernel -- the input gradient of BertOutput.dense pushed through BertIntermediate's activation."""
    M, K = gy.shape
    N = w.shape[1]
    assert tuple(h.shape) == (M, N) and h.is_contiguous()
    out = torch.empty((M, N), dtype=gy.dtype, device=gy.device)
    l = lib()
    t = TILES[tile]
    part = torch.empty((l.kvq_gemm_dgelu_partial_rows(M, t), N), dtype=torch.float32, device=gy.device)
    check(l.kvq_gemm_bf16_dgelu(gy.data_ptr(), w.data_ptr(), h.data_ptr(), out.data_ptr(), part.data_ptr(), part.numel() * 4, M, N, K,
                                gy.stride(0), w.stride(0), out.stride(0), t, stream_ptr()), "kvq_gemm_bf16_dgelu")
    return out, part


# ---- fp8 forward GEMMs (csrc/kvq_fp8.hip, kvq_gemm_fp8_nt) -----------------------------------------------------------------------
def gemm_ce(x, w, bias, V):
    """(logits, stats): logits = x @ w.T + bias [M, N] and the per-(row, 256-column tile) softmax statistics of the columns < V
    from the same kernel (LM head + forward half of the reconstruction loss; see ce_forward_stats)."""
    M, K = x.shape
    N = w.shape[0]
    logits = torch.empty((M, N), dtype=x.dtype, device=x.device)
    stats = torch.empty((M, (N + 255) // 256, 4), dtype=torch.float32, device=x.device)
    check(lib().kvq_gemm_bf16_ce(x.data_ptr(), w.data_ptr(), _p(bias), logits.data_ptr(), M, N, K, x.stride(0), w.stride(0),
                                 logits.stride(0), int(V), stats.data_ptr(), stats.numel() * 4, stream_ptr()), "kvq_gemm_bf16_ce")
    return logits, stats


# ---- the reconstruction loss (csrc/kvq_ce.hip).  Every pass has two entry points, kvq_X and kvq_X_ignore; these wrappers pick one:
# ignore_index=None is kvq_X, an int is kvq_X_ignore, whose means run over the rows whose target differs from it.  `count` [1] f32 on
# the device is their number: the forward passes write it (optional there), the backward passes read it (required).  No allocation
# and no synchronisation: the engine calls these while a step is being captured.
def _ce_ignore(who, ignore_index, count, count_required=False):
    """ignore_index as the int the _ignore entry point takes, or None for the entry point without it."""
    if ignore_index is None:
        if count is not None:
            raise KvqError(f"{who}: count is only used together with an ignore_index")
        return None
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, int):
        raise KvqError(f"{who}: ignore_index must be None or an int, got {ignore_index!r}")
    if count is None and count_required:
        raise KvqError(f"{who}: ignore_index={ignore_index} needs the count the forward pass wrote")
    return ignore_index


def ce_forward(logits, target, V, ld, row_loss, row_lse, pred, loss, acc, ignore_index=None, count=None):
    """Rows of V logits at stride ld -> row_loss, row_lse, pred [N] and the means loss, acc [1] (kvq_ce_forward / _ignore)."""
    ign = _ce_ignore("ce_forward", ignore_index, count)
    N = logits.shape[0]
    if ign is None:
        check(lib().kvq_ce_forward(logits.data_ptr(), target.data_ptr(), N, V, ld, io_dtype_of(logits), row_loss.data_ptr(),
                                   row_lse.data_ptr(), pred.data_ptr(), _p(loss), _p(acc), stream_ptr()), "kvq_ce_forward")
    else:
        check(lib().kvq_ce_forward_ignore(logits.data_ptr(), target.data_ptr(), N, V, ld, io_dtype_of(logits), ign, row_loss.data_ptr(),
                                          row_lse.data_ptr(), pred.data_ptr(), _p(loss), _p(acc), _p(count), stream_ptr()),
              "kvq_ce_forward_ignore")


def ce_forward_stats(logits, target, stats, row_loss, row_lse, pred, loss, acc, ignore_index=None, count=None):
    """ce_forward's outputs from gemm_ce()'s statistics (reads one logit per row; kvq_ce_forward_stats / _ignore)."""
    ign = _ce_ignore("ce_forward_stats", ignore_index, count)
    N = logits.shape[0]
    if ign is None:
        check(lib().kvq_ce_forward_stats(logits.data_ptr(), target.data_ptr(), N, logits.stride(0), io_dtype_of(logits), stats.data_ptr(),
                                         stats.shape[1], row_loss.data_ptr(), row_lse.data_ptr(), pred.data_ptr(), _p(loss), _p(acc),
                                         stream_ptr()), "kvq_ce_forward_stats")
    else:
        check(lib().kvq_ce_forward_stats_ignore(logits.data_ptr(), target.data_ptr(), N, logits.stride(0), io_dtype_of(logits),
                                                stats.data_ptr(), stats.shape[1], ign, row_loss.data_ptr(), row_lse.data_ptr(),
                                                pred.data_ptr(), _p(loss), _p(acc), _p(count), stream_ptr()),
              "kvq_ce_forward_stats_ignore")


def seq_acc(pred, target, B, S, per_sentence, ignore_index=None):
    """per_sentence [B] = the share of each sentence's S (counted) tokens with pred == target (kvq_seq_acc / _ignore)."""
    ign = _ce_ignore("seq_acc", ignore_index, None)
    if pred.numel() != B * S or target.numel() != B * S or per_sentence.numel() != B:
        raise KvqError(f"seq_acc: pred and target must hold {B} * {S} ids and per_sentence {B} values, got {pred.numel()}, "
                       f"{target.numel()} and {per_sentence.numel()}")
    if ign is None:
        check(lib().kvq_seq_acc(pred.data_ptr(), target.data_ptr(), B, S, per_sentence.data_ptr(), stream_ptr()), "kvq_seq_acc")
    else:
        check(lib().kvq_seq_acc_ignore(pred.data_ptr(), target.data_ptr(), B, S, ign, per_sentence.data_ptr(), stream_ptr()),
              "kvq_seq_acc_ignore")


def ce_backward(logits, target, row_lse, g_loss, V, ld, out, ignore_index=None, count=None):
    """out := g_loss * d mean(row_loss) / d logits, padding columns [V, ld) zero; out may be logits (kvq_ce_backward / _ignore).
    g_loss: [1] f32 on the device, or None for 1."""
    ign = _ce_ignore("ce_backward", ignore_index, count, count_required=True)
    N = logits.shape[0]
    if ign is None:
        check(lib().kvq_ce_backward(logits.data_ptr(), target.data_ptr(), row_lse.data_ptr(), _p(g_loss), N, V, ld, io_dtype_of(logits),
                                    out.data_ptr(), stream_ptr()), "kvq_ce_backward")
    else:
        check(lib().kvq_ce_backward_ignore(logits.data_ptr(), target.data_ptr(), row_lse.data_ptr(), _p(g_loss), count.data_ptr(), ign,
                                           N, V, ld, io_dtype_of(logits), out.data_ptr(), stream_ptr()), "kvq_ce_backward_ignore")


def ce_bwd_partial_rows(N):
    """Rows of ce_backward_bias's bias_part for N rows of logits: one per block of rows of the tiled kernel."""
    return lib().kvq_ce_bwd_partial_rows(N)


def ce_backward_bias(logits, target, row_lse, g_loss, V, ld, out, bias_part, ignore_index=None, count=None):
    """ce_backward with 16-byte aligned rows, which also leaves the column sums of out per block of rows in bias_part
    [kvq_ce_bwd_partial_rows(N), ld] f32 (kvq_ce_backward_bias / _ignore)."""
    ign = _ce_ignore("ce_backward_bias", ignore_index, count, count_required=True)
    N = logits.shape[0]
    if ign is None:
        check(lib().kvq_ce_backward_bias(logits.data_ptr(), target.data_ptr(), row_lse.data_ptr(), _p(g_loss), N, V, ld,
                                         io_dtype_of(logits), out.data_ptr(), bias_part.data_ptr(), bias_part.numel() * 4, stream_ptr()),
              "kvq_ce_backward_bias")
    else:
        check(lib().kvq_ce_backward_bias_ignore(logits.data_ptr(), target.data_ptr(), row_lse.data_ptr(), _p(g_loss), count.data_ptr(), ign,
                                                N, V, ld, io_dtype_of(logits), out.data_ptr(), bias_part.data_ptr(),
                                                bias_part.numel() * 4, stream_ptr()), "kvq_ce_backward_bias_ignore")


FP8_FORMATS = {"e4m3": FP8_E4M3, "e5m2": FP8_E5M2, FP8_E4M3: FP8_E4M3, FP8_E5M2: FP8_E5M2}


def _fp8_fmt(fmt):
    if fmt not in FP8_FORMATS:
        raise KvqError(f"fp8 format must be \"e4m3\" or \"e5m2\" (or _ffi.FP8_E4M3 / FP8_E5M2), got {fmt!r}")
    return FP8_FORMATS[fmt]


def fp8_quantize(x, out=None, fmt=None):
    """bf16 [rows, cols] (unit column stride) -> (fp8 bytes [rows, cols] as uint8, scale [1] f32 on the device).  fmt: None = e4m3
    through kvq_fp8_quantize (as before); "e4m3" / "e5m2": the format-taking entry kvq_fp8_quantize_fmt."""
    require_gpu(x)
    rows, cols = x.shape
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    st = torch.empty(2, dtype=torch.float32, device=x.device)             # [amax, scale]
    if fmt is None:
        check(lib().kvq_fp8_quantize(x.data_ptr(), rows, cols, x.stride(0), out.data_ptr(), st[0:].data_ptr(), st[1:].data_ptr(), stream_ptr()),
              "kvq_fp8_quantize")
    else:
        check(lib().kvq_fp8_quantize_fmt(x.data_ptr(), rows, cols, x.stride(0), out.data_ptr(), st[0:].data_ptr(), st[1:].data_ptr(),
                                         _fp8_fmt(fmt), stream_ptr()), "kvq_fp8_quantize_fmt")
    return out, st[1:]


def fp8_quantize_delayed(x, state, fmt, out=None, amax_only=False):
    """One pass over bf16 x [rows, cols]: the fp8 bytes (format fmt) under the scale state[0] of the delayed-scaling record `state`,
    this tensor's amax left in the record.  amax_only: nothing is written but the amax (returns None)."""
    require_gpu(x, state)
    rows, cols = x.shape
    if out is None and not amax_only:
        out = torch.empty((rows, cols), dtype=torch.uint8, device=x.device)
    check(lib().kvq_fp8_quantize_delayed_fmt(x.data_ptr(), rows, cols, x.stride(0), None if amax_only else out.data_ptr(), state.data_ptr(),
                                             _fp8_fmt(fmt), stream_ptr()), "kvq_fp8_quantize_delayed_fmt")
    return None if amax_only else out


def fp8_transpose(x8, out=None):
    """The byte transpose of an fp8 matrix held as uint8 [rows, cols] (unit column stride; rows, cols and the row stride multiples
    of 16): out [cols, rows] = x8.t(), dense."""
    require_gpu(x8)
    if x8.dim() != 2 or x8.element_size() != 1 or x8.stride(1) != 1:
        raise KvqError("fp8_transpose: a 2-d one-byte tensor with unit column stride")
    rows, cols = x8.shape
    if out is None:
        out = torch.empty((cols, rows), dtype=x8.dtype, device=x8.device)
    check(lib().kvq_fp8_transpose(x8.data_ptr(), rows, cols, x8.stride(0), out.data_ptr(), out.stride(0), stream_ptr()), "kvq_fp8_transpose")
    return out


def fp8_transpose_segments(src8, dst8, src_off, rows, cols, dst_off, max_tiles):
    """Dense fp8 matrices [rows[s], cols[s]] at src8 + src_off[s] -> their transposes at dst8 + dst_off[s], one launch (device int64
    tables, every entry a multiple of 16; max_tiles >= ceil(rows / 128) * ceil(cols / 128) of every segment)."""
    require_gpu(src8, dst8, src_off, rows, cols, dst_off)
    check(lib().kvq_fp8_transpose_segments(src8.data_ptr(), dst8.data_ptr(), src_off.data_ptr(), rows.data_ptr(), cols.data_ptr(),
                                           dst_off.data_ptr(), src_off.numel(), int(max_tiles), stream_ptr()), "kvq_fp8_transpose_segments")
    return dst8


def gemm_fp8_nt(a8, b8, scale_a, scale_b, bias=None, out=None, a_format=None, accumulate=False):
    """out[M,N] bf16 (+)= (a8[M,K] @ b8[N,K].T) / (scale_a * scale_b) + bias on the fp8 matrix cores.  a_format None, accumulate False:
    kvq_gemm_fp8_nt (both operands e4m3), as before; otherwise kvq_gemm_fp8_nt_ex with a8 in a_format ("e4m3" / "e5m2"; b8 is e4m3)
    and, with accumulate, the product added to the `out` that is there."""
    M, K = a8.shape
    N = b8.shape[0]
    if accumulate and out is None:
        raise KvqError("gemm_fp8_nt: accumulate needs the output to add to")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16, device=a8.device)
    if a_format is None and not accumulate:
        check(lib().kvq_gemm_fp8_nt(a8.data_ptr(), b8.data_ptr(), scale_a.data_ptr(), scale_b.data_ptr(), _p(bias), out.data_ptr(), M, N, K,
                                    a8.stride(0), b8.stride(0), out.stride(0), stream_ptr()), "kvq_gemm_fp8_nt")
    else:
        check(lib().kvq_gemm_fp8_nt_ex(a8.data_ptr(), b8.data_ptr(), scale_a.data_ptr(), scale_b.data_ptr(), _p(bias), out.data_ptr(), M, N, K,
                                       a8.stride(0), b8.stride(0), out.stride(0), _fp8_fmt("e4m3" if a_format is None else a_format),
                                       1 if accumulate else 0, stream_ptr()), "kvq_gemm_fp8_nt_ex")
    return out


def gemm_fp8_tile(M, N):
    """The name of the tile ("128x256" / "128x192") gemm_fp8_nt launches for an [M, N] output (kvq_gemm_fp8_tile: the launch's own rule)."""
    t = lib().kvq_gemm_fp8_tile(int(M), int(N))
    if t not in TILE_NAMES:
        raise KvqError(f"kvq_gemm_fp8_tile({M}, {N}) returned {t}")
    return TILE_NAMES[t]


def gemm_fp8_nt_gelu(a8, b8, scale_a, scale_b, bias, state_out=None):
    """(h, gelu(h)[, fp8 copy of gelu(h)]) with h = (a8 @ b8.T) / (scale_a * scale_b) + bias on the fp8 matrix cores: BertIntermediate
    with the GELU epilogue of gemm_gelu; state_out = the delayed-scaling record of the fp8 GEMM that reads gelu(h) next."""
    M, K = a8.shape
    N = b8.shape[0]
    h = torch.empty((M, N), dtype=torch.bfloat16, device=a8.device)
    a = torch.empty_like(h)
    a_8 = torch.empty((M, N), dtype=torch.uint8, device=a8.device) if state_out is not None else None
    check(lib().kvq_gemm_fp8_nt_gelu(a8.data_ptr(), b8.data_ptr(), scale_a.data_ptr(), scale_b.data_ptr(), _p(bias), h.data_ptr(),
                                     a.data_ptr(), _p(a_8), N if a_8 is not None else 0, _p(state_out), M, N, K, a8.stride(0), b8.stride(0),
                                     h.stride(0), stream_ptr()), "kvq_gemm_fp8_nt_gelu")
    return (h, a, a_8) if a_8 is not None else (h, a)


# ---- clock probe (bench.py) -----------------------------------------------------------------------------------------------------
def clock_probe():
    """Launch kvq_clock_probe on the current stream; returns its [rows, 4] int64 result buffer (read it after a synchronisation)."""
    l = lib()
    out = torch.zeros((l.kvq_clock_probe_rows(), 4), dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))
    check(l.kvq_clock_probe(out.data_ptr(), out.numel() * 8, stream_ptr()), "kvq_clock_probe")
    return out


def clock_mhz(p0, p1):
    """Shader clock held between two clock_probe() results of one stream: per XCD (the cycle counter is the XCD's own) the first
    stamp of each probe, d(s_memtime) / d(s_memrealtime) x 100 MHz; returns (median over the XCDs seen by both, {xcd: MHz})."""
    a, b = p0.cpu().tolist(), p1.cpu().tolist()

    def first(rows):
        d = {}
        for xcc, t, r, _ in rows:
            if xcc not in d or r < d[xcc][1]:
                d[xcc] = (t, r)
        return d
    fa, fb = first(a), first(b)
    per = {}
    for x in sorted(set(fa) & set(fb)):
        dt, dr = fb[x][0] - fa[x][0], fb[x][1] - fa[x][1]
        if dr > 0 and dt > 0:
            per[int(x)] = dt / dr * 100.0
    if not per:
        return None, {}
    v = sorted(per.values())
    return v[len(v) // 2], per


# ---- beam search (include/kvq.h "beam search"; csrc/kvq_generate.hip) ---------------------------------------------------------------
BEAM_MAX = 8


def _beam_anc(who, anc, R):
    if anc.dim() != 3 or anc.dtype != torch.int32 or anc.shape[0] != 2 or anc.shape[1] != R or not anc.is_contiguous():
        raise KvqError(f"kvq.nnops.{who}: the ancestry table must be a contiguous int32 [2, R = {R}, Lmax] tensor")
    return anc.shape[2]


def beam_attn_self(state, q, k_new, v_new, cache, anc, nh, out=None):
    """gen_attn_self in slot space: row r stores its k_new | v_new to cache row (r, t) and attends over keys 0 .. t, key j < t read
    from cache row (anc[t & 1][r, j], j) -- the beam's history, never a copy of the cache.  anc [2, R, Lmax] int32."""
    require_gpu(q, k_new, v_new, cache, anc)
    R, W = q.shape[0], nh * 64
    ldq, ldn = _gen_rows("beam_attn_self", q, "q"), _gen_rows("beam_attn_self", k_new, "k_new")
    if _gen_rows("beam_attn_self", v_new, "v_new") != ldn or k_new.shape != (R, W) or v_new.shape != (R, W) or q.shape[1] != W:
        raise KvqError(f"kvq.nnops.beam_attn_self: q, k_new, v_new must be [R, {W}] and k_new, v_new share a row stride")
    if cache.dim() != 3 or cache.shape[0] != R or cache.shape[2] != 2 * W or not cache.is_contiguous() or cache.dtype != q.dtype:
        raise KvqError(f"kvq.nnops.beam_attn_self: the cache must be a contiguous [R, Smax, {2 * W}] tensor of q's dtype")
    if _beam_anc("beam_attn_self", anc, R) < cache.shape[1]:
        raise KvqError("kvq.nnops.beam_attn_self: the ancestry table holds fewer positions than the cache")
    if out is None:
        out = torch.empty((R, W), dtype=q.dtype, device=q.device)
    check(lib().kvq_beam_attn(_gen_ptr(state), q.data_ptr(), ldq, k_new.data_ptr(), v_new.data_ptr(), ldn, cache.data_ptr(), cache.stride(1),
                              cache.stride(0), R, nh, 1, 0, cache.shape[1], anc.data_ptr(), anc.shape[2], 1, io_dtype_of(q), out.data_ptr(),
                              _gen_rows("beam_attn_self", out, "out"), stream_ptr()), "kvq_beam_attn")
    return out


def beam_attn_cross(state, q, kv, n_keys, nh, rows_per_sentence, out=None):
    """gen_attn_cross for rows_per_sentence query rows a sentence: row r of q [R, nh 64] reads the n_keys rows of sentence
    r // rows_per_sentence of kv [sentences * n_keys, 2 nh 64], sentences >= ceil(R / rows_per_sentence)."""
    require_gpu(q, kv)
    R, W, rps = q.shape[0], nh * 64, int(rows_per_sentence)
    ldq, ldk = _gen_rows("beam_attn_cross", q, "q"), _gen_rows("beam_attn_cross", kv, "kv")
    if rps < 1 or q.shape[1] != W or kv.shape[1] != 2 * W or kv.dtype != q.dtype or kv.shape[0] % n_keys \
            or kv.shape[0] // n_keys < -(-R // rps):
        raise KvqError(f"kvq.nnops.beam_attn_cross: q [R, {W}] needs kv [>= ceil(R / rows_per_sentence) * n_keys, {2 * W}] of its dtype, "
                       f"got {tuple(kv.shape)}")
    if out is None:
        out = torch.empty((R, W), dtype=q.dtype, device=q.device)
    check(lib().kvq_beam_attn(_gen_ptr(state), q.data_ptr(), ldq, None, None, 0, kv.data_ptr(), ldk, int(n_keys) * ldk, R, nh, 0, int(n_keys), 0,
                              None, 0, rps, io_dtype_of(q), out.data_ptr(), _gen_rows("beam_attn_cross", out, "out"), stream_ptr()),
          "kvq_beam_attn")
    return out


def _beam_rows(who, R, Lmax, **named):
    for name, (x, dtype, shape) in named.items():
        if x.dtype != dtype or tuple(x.shape) != shape or not x.is_contiguous():
            raise KvqError(f"kvq.nnops.{who}: {name} must be a contiguous {dtype} {shape} tensor")


def beam_select(state, logits, V, W, ids, parent, scores, step_scores, anc, finished, lengths, step_logits=None):
    """One step of beam search over logits [R, ld] in slot space (rows b W .. b W + W - 1 = sentence b): the W best of the live
    beams' V continuations and the finished beams themselves become the new beams -- token, parent, score, end-token bookkeeping
    and the extended ancestry rows (include/kvq.h).  t is read from the state; W = 1 .. 8."""
    require_gpu(logits, ids, parent, scores, step_scores, anc, finished, lengths)
    R = logits.shape[0]
    ld = _gen_rows("beam_select", logits, "logits")
    if ids.dim() != 2 or ids.dtype != torch.int64 or not ids.is_contiguous() or ids.shape[0] != R:
        raise KvqError("kvq.nnops.beam_select: ids must be a contiguous int64 [R, Lmax] tensor")
    Lmax = ids.shape[1]
    if _beam_anc("beam_select", anc, R) != Lmax:
        raise KvqError("kvq.nnops.beam_select: the ancestry table must be [2, R, Lmax]")
    _beam_rows("beam_select", R, Lmax, parent=(parent, torch.int32, (R, Lmax)), step_scores=(step_scores, torch.float32, (R, Lmax)),
               scores=(scores, torch.float32, (R,)), finished=(finished, torch.int32, (R,)), lengths=(lengths, torch.int32, (R,)))
    if step_logits is not None:
        _beam_rows("beam_select", R, Lmax, step_logits=(step_logits, torch.float32, (R, Lmax, V)))
    if isinstance(W, bool) or not isinstance(W, int) or not 1 <= W <= BEAM_MAX:
        raise KvqError(f"kvq.nnops.beam_select: W must be an int in 1 .. {BEAM_MAX}, got {W!r}")
    check(lib().kvq_beam_select(_gen_ptr(state), logits.data_ptr(), ld, int(V), R, W, Lmax, io_dtype_of(logits), ids.data_ptr(),
                                parent.data_ptr(), scores.data_ptr(), step_scores.data_ptr(), anc.data_ptr(), finished.data_ptr(),
                                lengths.data_ptr(), _p(step_logits), stream_ptr()), "kvq_beam_select")


def beam_gather(state, ids, anc, lengths, out=None):
    """out [R, Lmax] int64 = the hypotheses of the beams now living in the rows: out[r, j] = ids[anc[t & 1][r, j], j] for
    j < lengths[r], the state's pad id behind."""
    require_gpu(ids, anc, lengths)
    if ids.dim() != 2 or ids.dtype != torch.int64 or not ids.is_contiguous():
        raise KvqError("kvq.nnops.beam_gather: ids must be a contiguous int64 [R, Lmax] tensor")
    R, Lmax = ids.shape
    if _beam_anc("beam_gather", anc, R) != Lmax:
        raise KvqError("kvq.nnops.beam_gather: the ancestry table must be [2, R, Lmax]")
    _beam_rows("beam_gather", R, Lmax, lengths=(lengths, torch.int32, (R,)))
    if out is None:
        out = torch.empty_like(ids)
    elif out.dtype != torch.int64 or out.shape != ids.shape or not out.is_contiguous():
        raise KvqError("kvq.nnops.beam_gather: out must be a contiguous int64 [R, Lmax] tensor")
    check(lib().kvq_beam_gather(_gen_ptr(state), ids.data_ptr(), anc.data_ptr(), lengths.data_ptr(), R, Lmax, out.data_ptr(), stream_ptr()),
          "kvq_beam_gather")
    return out


# ---- free-running reconstruction metrics (include/kvq.h "free-running reconstruction metrics"; csrc/kvq_seqcmp.hip) ---------------
SEQ_COMPARE_MAX = 128         # tokens per side (csrc/kvq_seqcmp.hip SEQ_MAX)
SEQ_TABLE_MAX_ROWS, SEQ_TABLE_MAX_COLS = 4096, 16


def _seq_rows(who, name, x, B=None):
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.int64 or x.stride(1) != 1 or (B is not None and x.shape[0] != B):
        raise KvqError(f"kvq.nnops.{who}: {name} must be an int64 [B, L] tensor with unit column stride"
                       + (f" and B = {B}" if B is not None else ""))
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


def seq_compare(hyp, hyp_len, ref, ref_len, hyp_skip=0, Lmax=None, out=None, n_bad=None):
    """out [B, 4] int32 = (dist, hits, n, m) per sentence: the token edit distance (unit costs) and the positional matches of
    hyp[b, hyp_skip : hyp_len[b]] (n tokens) against ref[b, : ref_len[b]] (m tokens); hyp, ref int64 [B, L] (row strides are
    used), hyp_len, ref_len int32 [B].  Lmax (default: what the rows can hold) bounds n and m and is at most 128; a row with a
    length outside 0 .. Lmax, or past its row, gets (-1, 0, 0, 0) and adds 1 to n_bad (int64 [1] on the device, accumulated).
    Returns (out, n_bad); nothing is read back."""
    require_gpu(hyp, hyp_len, ref, ref_len)
    B = hyp.shape[0] if torch.is_tensor(hyp) and hyp.dim() == 2 else None
    ldh, ldr = _seq_rows("seq_compare", "hyp", hyp), _seq_rows("seq_compare", "ref", ref, B)
    for name, x in (("hyp_len", hyp_len), ("ref_len", ref_len)):
        if not torch.is_tensor(x) or x.dtype != torch.int32 or tuple(x.shape) != (B,) or not x.is_contiguous():
            raise KvqError(f"kvq.nnops.seq_compare: {name} must be a contiguous int32 [B] = [{B}] tensor")
    if isinstance(hyp_skip, bool) or not isinstance(hyp_skip, int):
        raise KvqError(f"kvq.nnops.seq_compare: hyp_skip must be an int, got {hyp_skip!r}")
    if Lmax is None:
        Lmax = max(hyp.shape[1] - max(hyp_skip, 0), ref.shape[1], 0)
    if out is None:
        out = torch.empty((B, 4), dtype=torch.int32, device=hyp.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (B, 4) or not out.is_contiguous():
        raise KvqError(f"kvq.nnops.seq_compare: out must be a contiguous int32 [B, 4] = [{B}, 4] tensor")
    if n_bad is None:
        n_bad = torch.zeros(1, dtype=torch.int64, device=hyp.device)
    elif n_bad.dtype != torch.int64 or n_bad.numel() != 1:
        raise KvqError("kvq.nnops.seq_compare: n_bad must be one int64 on the device")
    require_gpu(out, n_bad)
    check(lib().kvq_seq_compare(hyp.data_ptr(), ldh, hyp_skip, hyp_len.data_ptr(), ref.data_ptr(), ldr, ref_len.data_ptr(), B, int(Lmax),
                                out.data_ptr(), n_bad.data_ptr(), stream_ptr()), "kvq_seq_compare")
    return out, n_bad


def seq_compare_accumulate(per, slot, table):
    """table [R, 6] int64 += (1, dist == 0, dist, hits, n, m) of every sentence of per [B, 4] (seq_compare's out) with dist >= 0, at
    each row slot[b, c] (int32 [B, C]) inside [0, R); other slots are skipped.  Integer sums: the same bits in any order."""
    require_gpu(per, slot, table)
    if per.dim() != 2 or per.shape[1] != 4 or per.dtype != torch.int32 or not per.is_contiguous():
        raise KvqError("kvq.nnops.seq_compare_accumulate: per must be a contiguous int32 [B, 4] tensor")
    B = per.shape[0]
    if slot.dim() != 2 or slot.shape[0] != B or slot.dtype != torch.int32 or not slot.is_contiguous():
        raise KvqError(f"kvq.nnops.seq_compare_accumulate: slot must be a contiguous int32 [B, C] tensor with B = {B}")
    if table.dim() != 2 or table.shape[1] != 6 or table.dtype != torch.int64 or not table.is_contiguous():
        raise KvqError("kvq.nnops.seq_compare_accumulate: table must be a contiguous int64 [R, 6] tensor")
    check(lib().kvq_seq_compare_accumulate(per.data_ptr(), B, slot.data_ptr(), slot.shape[1], table.shape[0], table.data_ptr(),
                                           stream_ptr()), "kvq_seq_compare_accumulate")
    return table
