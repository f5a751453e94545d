"""f64 references and judges of the generation kernels (csrc/kvq_generate.hip) and of TrainEngine.generate -- the checkers of
tests/test_generate_kernels_gpu.py and tests/test_generate_engine_gpu.py.  Plain torch, no device needed.

attn_ref       softmax(q . k^T / 8) . v in f64 on the dtype-exact inputs (the upcast bf16 / f32 values), head layout
               q [B, nh, 64], k, v [B, nh, n, 64]  ->  (out [B, nh, 64], bound_term [B, nh, 64] = sum_j p_j |v_j|)
attn_judge     the bound of the issue, per (sentence, head, column):
                   |got - ref| <= r |ref| + 2^-16 sum_j p_j |v_j|,    r = 2^-8 for a bf16 output, 0 for f32
               r |ref|: the single rounding of the output (bf16 keeps 8 significant bits: half an ulp is 2^-8 of the value's power
               of two, hence at most 2^-8 of the value).  2^-16 sum p |v|: f32
               accumulation of at most 128 terms (128 * 2^-24 = 2^-17) plus the error of exp((s - max) log2 e) through the
               fast-exp argument scaling at |s - max| up to about 100 (100 * 1.44 * 2^-24 < 2^-16.8).  Derived, not tuned.
select_ref     the bookkeeping of kvq_gen_select on the host.
frequency_bound   5 sqrt(p (1 - p) / n): five standard deviations of a binomial frequency.
"""
from __future__ import annotations

import math

import torch

ATTN_ABS = 2.0 ** -16
ATTN_REL = {torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}


def attn_ref(q, k, v):
    q, k, v = q.double(), k.double(), v.double()
    s = torch.einsum("bhd,bhnd->bhn", q, k) / 8.0
    p = torch.softmax(s, dim=-1)
    return torch.einsum("bhn,bhnd->bhd", p, v), torch.einsum("bhn,bhnd->bhd", p, v.abs())


def attn_judge(got, ref, term, dtype):
    """-> (ok, worst ratio |got - ref| / bound).  A bound of 0 (an exactly zero reference with zero values) demands equality."""
    err = (got.double() - ref).abs()
    bound = ATTN_REL[dtype] * ref.abs() + ATTN_ABS * term
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    worst = float(ratio.max())
    return worst <= 1.0, worst


def heads(x, nh):
    """[B, nh * 64] or [B, n, nh * 64] -> [B, nh, 64] / [B, nh, n, 64]"""
    if x.dim() == 2:
        return x.reshape(x.shape[0], nh, 64)
    return x.reshape(x.shape[0], x.shape[1], nh, 64).permute(0, 2, 1, 3)


def select_ref(choice, ids, finished, lengths, t, P, eos_id, pad_id):
    """One step of kvq_gen_select's bookkeeping on host tensors (modified in place): choice [B] = the arg-max of the step."""
    Lmax = ids.shape[1]
    if t + 1 >= Lmax or t + 1 < P:
        return
    for b in range(ids.shape[0]):
        if finished[b]:
            ids[b, t + 1] = pad_id
        else:
            ids[b, t + 1] = int(choice[b])
            if eos_id is not None and int(choice[b]) == eos_id:
                finished[b] = 1
                lengths[b] = t + 2


def frequency_bound(p, n):
    return 5.0 * torch.sqrt(p * (1.0 - p) / n)
