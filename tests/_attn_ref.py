"""f64 reference, rounding model and per-row judge of the bf16 attention kernels (csrc/kvq_nn.hip) -- the checker of
tests/test_attn_parity_gpu.py; tests/test_attn_ref.py checks the checker itself without a GPU.

All tensors are in head layout: q, g_out, ctx, g_q [B, nh, Sq, 64]; k, v, g_k, g_v [B, nh, Sk, 64]; lse [B, nh, Sq]; keep
[B, nh, Sq, Sk] (0 / 1, None = no dropout); mask [B, Sk] (1 = attend) or None; bias partials [B, nh, 64].

reference() is BertSelfAttention / cross-attention math (modeling_bert.py:111-204) in f64 on the upcast bf16 inputs, with the
conventions of tests/_dropout_ref.py::ref_step (it calls the same helpers): additive key mask, keep / (1 - p) on the
probabilities.  One thing is defined here that torch leaves NaN: a query row without any attended key has all-zero
probabilities, output 0 and lse = log(1e-37), the contract include/kvq.h states for kvq_attn_fwd.

model() is the same computation with the roundings the kernels document and nothing else different: f32 summation order and the
exp / log / reciprocal implementations are NOT restated (the 2x of the margins covers them).  `family`:
  "mfma"  attn_fwd_mfma_kernel / attn_bwd_mfma_kernel (at most 32 tokens on either side)
  "blk"   attn_fwd_blk_kernel / attn_bwd_blk_dq_kernel / attn_bwd_blk_dkv_kernel (33 .. 128 tokens, 32-key blocks)
Rounding points (csrc/kvq_nn.hip; line numbers of the commit that added this file):
  R1  P~ = bf16(P * keep / (1 - p)) before P~.V             acc_to_frags():1861 from attn_fwd_mfma_kernel:2026-2028
      blk: bf16(exp(s - running max) * keep / (1 - p)), per key block, NOT normalised   attn_fwd_blk_kernel:2286-2294
  R2  every output row is rounded to bf16 on store          store_rows_coalesced():1915-1916, store_ct():1891-1892
  R3  dS = bf16(P (dP~ keep/(1-p) - delta) scale) before dS.K and dS^T.Q   acc_to_frags():1861, stage_transposed():1870
      (attn_bwd_mfma_kernel:2111-2117; blk_grad_pair():2331)
  R4  P~ = bf16(P keep/(1-p)) before P~^T.dO                stage_transposed():1870 (attn_bwd_mfma_kernel:2112-2115;
      blk_grad_pair():2332)
  R5  mfma: delta = sum_j P dP~ keep/(1-p) with the UNROUNDED f32 P                  attn_bwd_mfma_kernel:2103-2107
      blk : delta = rowsum(g_out * out) from the STORED bf16 forward output          blk_row_dot():2233, :2350, :2403
  R6  blk : P = exp(s - lse) from the STORED f32 lse                                 blk_grad_pair():2330
  R7  bias partials.  mfma: K . colsum(bf16 dS), Q . rowsum(bf16 dS), dO . rowsum(bf16 P~) in f32, i.e. the column sums of the
      f32 gradients BEFORE R2 (attn_bwd_mfma_kernel:2139-2154, :2167, :2179).  blk: a column-sum pass over the stored
      (R2-rounded) gradients (attn_bias_partials():3000).
Scores and dP~ are f32 accumulations of exact bf16 products: no rounding point.
"""
from __future__ import annotations

import math

import torch

from _dropout_ref import attend_allowed, dropout_scale, masked_softmax

LSE_EMPTY = math.log(1e-37)      # lse of a query row that attends to nothing (kvq_nn.hip scores_to_probs():1425, :2312)

# lse is an f32 output with no bf16 rounding anywhere behind it: scores are f32 sums of 64 exact products (error <= 64 * 2^-24 *
# sum_d |q_d k_d| * scale, about 2^-16 for randn operands), v_exp_f32 / v_log_f32 are 1-ulp instructions whose argument scaling
# by log2(e) costs |s - max| * 2^-24 relative (|s - max| < 16 for every term that matters: 2^-20), and the result is rounded to
# f32 at a magnitude below 8 (2^-22), below 128 for an empty row (2^-18 relative to LSE_EMPTY).
LSE_ATOL = 2.0 ** -15
LSE_RTOL = 2.0 ** -20


def rbf(x):
    """round to bf16 (nearest even, through f32 as the kernels do) and back to x's dtype"""
    return x.float().bfloat16().to(x.dtype)


def _id(x):
    return x


def _lse(s, allow):
    sm = s.masked_fill(~allow, float("-inf"))
    some = allow.any(-1)
    out = torch.logsumexp(torch.where(some[..., None], sm, torch.zeros_like(sm)), -1)
    return torch.where(some, out, torch.full_like(out, LSE_EMPTY))


def _colsum(g):
    return g.sum(2)                                     # [B, nh, S, 64] -> [B, nh, 64]


def reference(q, k, v, mask, causal, scale, keep, p, g_out):
    """f64, autograd.  dict(ctx, lse, g_q, g_k, g_v, pb_q, pb_k, pb_v); pb_* = per-sentence column sums of the bf16-rounded
    gradients (`as stored`: include/kvq.h on bias_part_*)."""
    B, nh, Sq, _ = q.shape
    Sk = k.shape[2]
    q, k, v = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    allow = attend_allowed(B, Sq, Sk, mask, causal, q.device).expand(B, nh, Sq, Sk)
    s = q @ k.transpose(-1, -2) * scale
    pr = masked_softmax(s, allow, empty_rows_zero=True)
    if keep is not None:
        pr = dropout_scale(pr, keep, p)
    ctx = pr @ v
    ctx.backward(g_out.double())
    out = dict(ctx=ctx.detach(), lse=_lse(s.detach(), allow), g_q=q.grad, g_k=k.grad, g_v=v.grad)
    for n in "qkv":
        out["pb_" + n] = _colsum(rbf(out["g_" + n]))
    return out


def model(q, k, v, mask, causal, scale, keep, p, g_out, family="mfma", rounding=True, hooks=None):
    """The kernels' computation in f64 with their rounding points (module docstring); rounding=False switches every one of
    them off (then model == reference to f64 noise).  hooks: {name: function} applied to the named intermediate -- how
    tests/test_attn_ref.py plants the bugs of mutations(): "allow" [B, nh, Sq, Sk] bool, "keep" [B, nh, Sq, Sk],
    "delta_keep" (the keep scale inside delta only).  Returns reference()'s dict."""
    assert family in ("mfma", "blk")
    hooks = hooks or {}
    rnd = rbf if rounding else _id
    B, nh, Sq, _ = q.shape
    Sk = k.shape[2]
    q, k, v, g = (t.detach().double() for t in (q, k, v, g_out))
    allow = hooks.get("allow", _id)(attend_allowed(B, Sq, Sk, mask, causal, q.device).expand(B, nh, Sq, Sk).clone())
    if keep is not None:
        keep = hooks.get("keep", _id)(keep.clone())
    ks = torch.ones(B, nh, Sq, Sk, dtype=torch.float64, device=q.device)
    if keep is not None:
        ks = dropout_scale(ks, keep, p)
    ks_delta = hooks.get("delta_keep", _id)(ks)
    s_raw = q @ k.transpose(-1, -2) * scale
    s = s_raw.masked_fill(~allow, float("-inf"))
    some = allow.any(-1, keepdim=True)
    lse = _lse(s, allow)
    if family == "mfma":
        P = masked_softmax(s_raw, allow, empty_rows_zero=True)
        ctx_acc = rnd(P * ks) @ v                                                    # R1
    else:
        m_run = torch.full((B, nh, Sq, 1), float("-inf"), dtype=torch.float64, device=q.device)
        l_run = torch.zeros_like(m_run)
        o = torch.zeros(B, nh, Sq, 64, dtype=torch.float64, device=q.device)
        for k0 in range(0, Sk, 32):                                                  # attn_fwd_blk_kernel:2261-2303
            sb = s[..., k0:k0 + 32]
            m_new = torch.maximum(m_run, sb.amax(-1, keepdim=True))
            mref = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)
            alpha = torch.exp(m_run - mref)
            e = torch.exp(sb - mref)
            l_run = l_run * alpha + e.sum(-1, keepdim=True)
            o = o * alpha + rnd(e * ks[..., k0:k0 + 32]) @ v[:, :, k0:k0 + 32]       # R1 (blk)
            m_run = m_new
        ctx_acc = torch.where(l_run > 0, o / l_run.clamp_min(1e-300), torch.zeros_like(o))
    ctx = rnd(ctx_acc)                                                               # R2
    dpt = g @ v.transpose(-1, -2)
    if family == "mfma":
        delta = (P * dpt * ks_delta).sum(-1, keepdim=True)                           # R5 (mfma)
    else:
        lse_st = lse.float().double() if rounding else lse                           # R6
        P = torch.where(allow, torch.exp(s - lse_st[..., None]), torch.zeros_like(s))
        if "delta_keep" in hooks:
            delta = (P * dpt * ks_delta).sum(-1, keepdim=True)
        else:
            delta = (g * ctx).sum(-1, keepdim=True)                                  # R5 (blk)
        delta = delta * some
    dS = rnd(P * (dpt * ks - delta) * scale)                                         # R3
    Pt = rnd(P * ks)                                                                 # R4
    acc = dict(g_q=dS @ k, g_k=dS.transpose(-1, -2) @ q, g_v=Pt.transpose(-1, -2) @ g)
    out = dict(ctx=ctx, lse=lse)
    for n, a in acc.items():
        out[n] = rnd(a)                                                              # R2
        out["pb_" + n[-1]] = _colsum(a if family == "mfma" else out[n])              # R7
    return out


def worst_ratio(got, ref, mod, zero_floor=None):
    """max over elements of |got - ref| / env(row), env(row) = max_d |mod - ref| + 2^-9 max_d |ref| over the row's last
    dimension; returns (ratio, index tuple of the worst element).  0 / 0 counts as 0 (an exactly-zero row met exactly).
    zero_floor (broadcastable to the rows): added to env ONLY where the reference row is exactly zero, see cancellation_floors()."""
    got, ref, mod = got.double(), ref.double(), mod.double()
    rmax = ref.abs().amax(-1, keepdim=True)
    env = (mod - ref).abs().amax(-1, keepdim=True) + 2.0 ** -9 * rmax
    if zero_floor is not None:
        env = env + torch.where(rmax == 0, zero_floor.expand_as(rmax), torch.zeros_like(rmax))
    diff = (got - ref).abs()
    diff = torch.where(torch.isfinite(diff), diff, torch.full_like(diff, float("inf")))          # NaN counts as a miss
    ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / env.expand_as(diff))
    flat = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
    return float(ratio.reshape(-1)[flat]), idx


def cancellation_floors(q, k, v, g_out, mask, causal, scale):
    """Rows whose exact gradient is ZERO by cancellation -- a query i with a single attended key j* has P = 1 and
    dS = P (dP - delta) scale = 0 -- leave env(row) = 0, and the relative envelope says nothing there.  The blocked kernels
    form dP (MFMA accumulator, blk_grad_pair():2324) and delta (fma chain over g_out * out, blk_row_dot():2240) as two separately
    ordered 64-term f32 sums, so their difference is f32 summation noise instead of 0; the 32-token kernel takes delta from the
    same dP (attn_bwd_mfma_kernel:2105) and does give exact zeros.  Per-row bound (n-term f32 dot product: error <=
    n 2^-24 sum |x_i y_i|, once for dP and once for delta), for the pairs (i, j*) of single-key queries only:
        e[i]        = scale * 2 * 64 * 2^-24 * sum_d |g_id v_j*d|           (|dS[i][j*]| <= e[i])
        g_q row i  <= e[i] * max_d |k_j*d|
        g_k row j  <= sum over the single-key queries i of j:  e[i] * max_d |q_id|
        partials   <= the sum of their sentence's row floors.
    About 1e-4 for randn operands.  Returns {name: [B, nh, S, 1] or [B, nh, 1]} for judge_all(floors=...); used for the blocked
    family only, and added only on rows whose reference is exactly zero (worst_ratio): every other row keeps the envelope."""
    q, k, v, g = (t.double().abs() for t in (q, k, v, g_out))
    B, nh, Sq, _ = q.shape
    Sk = k.shape[2]
    allow = attend_allowed(B, Sq, Sk, mask, causal, q.device).expand(B, nh, Sq, Sk)
    single = allow & (allow.sum(-1, keepdim=True) == 1)                               # the pairs (i, j*)
    e = scale * 2 * 64 * 2.0 ** -24 * (g @ v.transpose(-1, -2)) * single              # [B, nh, Sq, Sk]
    fq = (e * k.amax(-1)[:, :, None, :]).sum(-1, keepdim=True)                        # [B, nh, Sq, 1]
    fk = (e * q.amax(-1)[:, :, :, None]).sum(2)[..., None]                            # [B, nh, Sk, 1]
    return {"g_q": fq, "g_k": fk, "pb_q": fq.sum(2), "pb_k": fk.sum(2)}


def judge(got, ref, mod, unit, margin=1.0, zero_floor=None):
    """Per row of a unit one workgroup produces -- (sentence, head, query or key row) over its 64 columns, (sentence, head) for
    a bias partial: assert |got - ref| <= margin * env(row) for every element.  `unit` names the tensor in the report.
    Returns the worst ratio |got - ref| / env."""
    assert got.shape == ref.shape == mod.shape, (unit, tuple(got.shape), tuple(ref.shape), tuple(mod.shape))
    ratio, idx = worst_ratio(got, ref, mod, zero_floor)
    where = dict(zip(("sentence", "head", "row", "column") if len(idx) == 4 else ("sentence", "head", "column"), idx))
    assert ratio <= margin, f"{unit}: worst |got - ref| / env = {ratio:.3f} > margin {margin} at {where}"
    return ratio


def judge_lse(got, ref, unit="lse"):
    """lse is an f32 output: elementwise |got - ref| <= LSE_ATOL + LSE_RTOL |ref|.  Returns the worst |got - ref| / tolerance."""
    got, ref = got.double(), ref.double()
    diff = (got - ref).abs()
    diff = torch.where(torch.isfinite(diff), diff, torch.full_like(diff, float("inf")))
    ratio = diff / (LSE_ATOL + LSE_RTOL * ref.abs())
    flat = int(ratio.argmax())
    idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
    worst = float(ratio.reshape(-1)[flat])
    assert worst <= 1.0, f"{unit}: |got - ref| = {float(diff.reshape(-1)[flat]):.3e} is {worst:.2f} x the f32 tolerance at (sentence, head, row) {idx}"
    return worst


OUTPUTS = ("ctx", "g_q", "g_k", "g_v", "pb_q", "pb_k", "pb_v")
FAMILY_OF = {"ctx": "fwd", "g_q": "bwd", "g_k": "bwd", "g_v": "bwd", "pb_q": "bwd", "pb_k": "bwd", "pb_v": "bwd"}


def judge_all(got, ref, mod, margins, label="", report=None, floors=None):
    """judge() every output of OUTPUTS plus the lse; margins {"fwd": m, "bwd": m}.  Returns {name: worst ratio}; raises after all
    outputs have been looked at and report(label, ratios) has been called, so that a failing run still shows every figure."""
    ratios, errors = {}, []
    for name in OUTPUTS:
        if name not in got:
            continue
        try:
            ratios[name] = judge(got[name], ref[name], mod[name], f"{label} {name}", margins[FAMILY_OF[name]], (floors or {}).get(name))
        except AssertionError as e:
            ratios[name] = worst_ratio(got[name], ref[name], mod[name], (floors or {}).get(name))[0]
            errors.append(str(e))
    if "lse" in got:
        try:
            ratios["lse"] = judge_lse(got["lse"], ref["lse"], f"{label} lse")
        except AssertionError as e:
            ratios["lse"] = float("inf")
            errors.append(str(e))
    if report is not None:
        report(label, ratios)
    assert not errors, "\n".join(errors)
    return ratios


# ---- mutations: what a plausible kernel bug would have produced, built from the model's intermediates or outputs ------------------
# Each entry: name -> function(case) -> mutated model output dict, or None when the case cannot show the bug (e.g. no dropout).
# `case` is a dict(q, k, v, mask, causal, scale, keep, p, g_out, family); b, h pick the (sentence, head) that is hit.

def _last_attended(mask, b, Sk):
    return Sk - 1 if mask is None else int(torch.nonzero(mask[b]).max())


def _run(case, hooks=None):
    return model(case["q"], case["k"], case["v"], case["mask"], case["causal"], case["scale"], case["keep"], case["p"], case["g_out"],
                 family=case["family"], hooks=hooks)


def mut_last_key_left_out(case, b=1, h=1):
    j = _last_attended(case["mask"], b, case["k"].shape[2])

    def f(allow):
        allow[b, h, :, j] = False
        return allow
    return _run(case, {"allow": f})


def mut_first_padded_key_attended(case, b=1, h=1):
    mask = case["mask"]
    if mask is None or bool(mask[b].all()):
        return None
    j = int(torch.nonzero(mask[b] == 0).min())
    if case["causal"] and j >= case["q"].shape[2]:
        return None

    def f(allow):
        allow[b, h, :, j] = True
        if case["causal"]:
            allow[b, h, :j, j] = False
        return allow
    return _run(case, {"allow": f})


def mut_causal_edge_off_by_one(case):
    if not case["causal"]:
        return None
    Sq, Sk = case["q"].shape[2], case["k"].shape[2]

    def f(allow):                                          # key <= query + 1 instead of key <= query
        edge = torch.ones(Sq, Sk, dtype=torch.bool, device=allow.device).tril(1)
        keyok = torch.ones_like(allow) if case["mask"] is None else case["mask"].bool()[:, None, None, :].expand_as(allow)
        return keyok & edge
    return _run(case, {"allow": f})


def mut_keep_transposed(case, b=1, h=1):
    if case["keep"] is None or case["q"].shape[2] != case["k"].shape[2]:
        return None

    def f(keep):
        keep[b, h] = keep[b, h].t().clone()
        return keep
    return _run(case, {"keep": f})


def mut_delta_without_keep(case):
    if case["keep"] is None:
        return None
    return _run(case, {"delta_keep": torch.ones_like})


def mut_scale_missing_on_g_k(case):
    out = dict(_run(case))
    out["g_k"] = out["g_k"] / case["scale"]                 # scale = 1/8: a power of two commutes with the rounding
    out["pb_k"] = out["pb_k"] / case["scale"]
    return out


def mut_heads_swapped_in_g_v(case, h0=0, h1=2):
    out = dict(_run(case))
    gv = out["g_v"].clone()
    gv[:, [h0, h1]] = gv[:, [h1, h0]]
    out["g_v"] = gv
    return out


def _mut_row_scaled(name):
    def f(case, b=2, h=1):
        out = dict(_run(case))
        t = out[name].clone()
        row = t.shape[2] - 1 if name in ("ctx", "g_q") else 0        # (causal: query 0 has g_q = 0, key 0 is always attended)
        t[b, h, row] = rbf(t[b, h, row] * (1 + 2.0 ** -4))
        out[name] = t
        return out
    return f


def _mut_partial_loses_last_token(n):
    def f(case, b=2):
        out = dict(_run(case))
        S = out["g_" + n].shape[2]
        last = S - 1 if n == "q" else min(_last_attended(case["mask"], b, S), S - 1)
        if n != "q" and case["causal"]:
            last = min(last, case["q"].shape[2] - 1)
        t = out["pb_" + n].clone()
        t[b] = t[b] - out["g_" + n][b, :, last]
        out["pb_" + n] = t
        return out
    return f


MUTATIONS = {
    "last attended key left out": mut_last_key_left_out,
    "first padded key attended": mut_first_padded_key_attended,
    "causal edge off by one": mut_causal_edge_off_by_one,
    "keep mask transposed": mut_keep_transposed,
    "delta without the keep mask": mut_delta_without_keep,
    "scale missing on g_k": mut_scale_missing_on_g_k,
    "heads swapped in g_v": mut_heads_swapped_in_g_v,
    "ctx row times 1 + 2^-4": _mut_row_scaled("ctx"),
    "g_q row times 1 + 2^-4": _mut_row_scaled("g_q"),
    "g_k row times 1 + 2^-4": _mut_row_scaled("g_k"),
    "g_v row times 1 + 2^-4": _mut_row_scaled("g_v"),
    "pb_q loses its last token": _mut_partial_loses_last_token("q"),
    "pb_k loses its last token": _mut_partial_loses_last_token("k"),
    "pb_v loses its last token": _mut_partial_loses_last_token("v"),
}

# the output on which each mutation must exceed the margin by the per-row envelope itself (not through the lse check)
MUTATION_TARGET = {
    "last attended key left out": "ctx", "first padded key attended": "ctx", "causal edge off by one": "ctx",
    "keep mask transposed": "ctx", "delta without the keep mask": "g_q", "scale missing on g_k": "g_k", "heads swapped in g_v": "g_v",
    "ctx row times 1 + 2^-4": "ctx", "g_q row times 1 + 2^-4": "g_q", "g_k row times 1 + 2^-4": "g_k", "g_v row times 1 + 2^-4": "g_v",
    "pb_q loses its last token": "pb_q", "pb_k loses its last token": "pb_k", "pb_v loses its last token": "pb_v",
}

# ---- margins: one per kernel family, at most 2 x the largest worst ratio of one run on the MI355X ----------------------------------
# (tests/test_attn_parity_gpu.py prints every case's figures).  Measured worst |got - ref| / env per case class, forward | backward
# (rows and bias partials) | lse against its f32 tolerance:
#   32-token MFMA kernels   step shape B=256 nh=12 S=32      0.799 | 1.163 | 0.017
#                           cross-attention, engine layout   0.785 | 1.030 | 0.020
#                           ragged / holes / single          0.770 | 0.999 | 0.066
#                           sentence without a key           0.747 | 1.001 | 0.066
#   blocked kernels         33 .. 128 tokens B=64 nh=12      1.063 | 1.540 | 0.022
#                           sentence without a key           0.748 | 1.000 | 0.066
# Nothing above 3; the model is faithful (ratios near 1).  One finding on the way: with no dropout a query that attends a single key
# has g_q = g_k = 0 exactly, the blocked backward returns f32 summation noise there -- see cancellation_floors(): a per-row
# bound of about 1e-4, added on exactly-zero reference rows only; the figures above include those rows.
MARGIN = {
    "mfma": {"fwd": 1.5, "bwd": 2.0},
    "blk": {"fwd": 2.0, "bwd": 3.0},
}
