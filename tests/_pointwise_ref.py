"""f64 / integer references, case generators and judges for the reduction, GELU and reconstruction-loss kernels
(tests/test_reduce_exact_gpu.py, test_gelu_parity_gpu.py, test_ce_parity_gpu.py).  Everything here runs on the CPU;
tests/test_pointwise_ref.py shows that each judge accepts a plain f32 / bf16 restatement and rejects planted mistakes."""
import functools
import math

import torch

EXACT_LIMIT = 1 << 24          # integers (and half-integers times two) below this are exact in f32
INT_MAX = 2147483647


# ---------------------------------------------------------------------------------------------------------------
# exact integer cases for the reductions
# ---------------------------------------------------------------------------------------------------------------
def int_values(shape, seed):
    """int64 values in [-8, 8] without 0 (exact in bf16 and f32): a dropped or doubled row changes EVERY column."""
    g = torch.Generator().manual_seed(int(seed))
    v = torch.randint(1, 9, shape, generator=g)
    s = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return v * s


def assert_exact_range(*refs):
    """The condition under which f32 accumulation in any grouping is exact: every value (times two, for scale 0.5) is an
    integer below 2^24.  Checked on the CPU, on the reference."""
    for r in refs:
        r2 = 2.0 * r.double()
        assert torch.all(r2 == torch.round(r2)) and float(r2.abs().max()) < EXACT_LIMIT, "integer case leaves the exact f32 range"


def reduce_ref(src, scale=1.0, dst0=None):
    """dst[c] = scale * sum_p src[p, c] (+ dst0[c]) on int64 sources; f64 result, exact."""
    assert src.dtype == torch.int64
    s = src.sum(0)
    assert_exact_range(s)
    out = s.double() * float(scale)
    if dst0 is not None:
        out = out + dst0.double()
    assert_exact_range(out)
    return out


def block_sums(x, rows):
    """Partial rows of a blocked column sum: part[b] = sum of rows [b*rows, (b+1)*rows) of int64 x [N, C]."""
    N = x.shape[0]
    out = torch.stack([x[r:r + rows].sum(0) for r in range(0, N, rows)])
    assert_exact_range(out)
    return out.double()


def bf16_bits(t):
    return t.contiguous().view(torch.int16)


def judge_exact(out, ref):
    """out (f32 or bf16, any device) against the exact f64 reference: f32 equal by value; bf16 bitwise equal to the single RNE
    rounding of the exact value.  -0 and +0 are equal.  Returns the number of mismatches."""
    out = out.detach().cpu()
    ref = ref.double().reshape(out.shape)
    if out.dtype == torch.float32:
        return int((out.double() != ref).sum())
    assert out.dtype == torch.bfloat16
    want = ref.float().bfloat16()                       # ref is exact in f32 (assert_exact_range), so this rounds once, RNE
    same = (bf16_bits(out) == bf16_bits(want)) | ((out.float() == 0) & (want.float() == 0))
    return int((~same).sum())


# ---------------------------------------------------------------------------------------------------------------
# GELU (erf form)
# ---------------------------------------------------------------------------------------------------------------
SQRT1_2 = 0.70710678118654752
INV_SQRT_2PI = 0.39894228040143268


def all_bf16_values():
    """All 65536 bf16 bit patterns as a bf16 tensor (a multiple of 8 long), and the mask of the finite ones."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    x = bits.view(torch.bfloat16)
    return x, torch.isfinite(x.float())


def gelu_ref(x):
    """f64 x * Phi(x) and Phi(x) + x * phi(x) of the up-cast input; erfc keeps the negative tail accurate."""
    x = x.double()
    cdf = 0.5 * torch.special.erfc(-x * SQRT1_2)
    pdf = INV_SQRT_2PI * torch.exp(-0.5 * x * x)
    return x * cdf, cdf + x * pdf


def as_cdf_f64(x):
    """The bf16 kernels' formula (Abramowitz & Stegun 7.1.26) in f64: Phi(x) and exp(-x^2/2)."""
    x = x.double()
    z = x.abs() * SQRT1_2
    t = 1.0 / (1.0 + 0.3275911 * z)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    e = torch.exp(-z * z)
    half_tail = 0.5 * poly * e
    return torch.where(x >= 0, 1.0 - half_tail, half_tail), e


@functools.lru_cache(maxsize=None)
def gelu_delta():
    """delta of the bf16 envelopes: twice the worst error of the A&S formula on the CDF, the formula evaluated in f64 against
    f64 erfc over every finite bf16 value and a dense grid (the other half is for the kernel's f32 rcp, polynomial and exp).
    Returns (delta, worst error, x of the worst error)."""
    xs, fin = all_bf16_values()
    x = torch.cat([xs.double()[fin], torch.linspace(-10.0, 10.0, 2_000_001, dtype=torch.float64)])
    err = (as_cdf_f64(x)[0] - 0.5 * torch.special.erfc(-x * SQRT1_2)).abs()
    i = int(err.argmax())
    return 2.0 * float(err[i]), float(err[i]), float(x[i])


TINY = 2.0 ** -126


def gelu_bf16_ratio(out, x, ref, backward):
    """|out - ref| over the bf16 envelope 2^-8 |ref| + delta (|x| or 1 + |x|) + 2^-126, per element (<= 1 passes)."""
    d = gelu_delta()[0]
    x = x.double()
    env = ref.abs() * 2.0 ** -8 + d * ((1.0 + x.abs()) if backward else x.abs()) + TINY
    return (out.detach().cpu().double() - ref).abs() / env


def f32_ratio(out, ref, rtol=1e-5, atol=1e-5):
    """|out - ref| / (atol + rtol |ref|) per element."""
    return (out.detach().cpu().double() - ref).abs() / (atol + rtol * ref.abs())


# ---------------------------------------------------------------------------------------------------------------
# reconstruction loss
# ---------------------------------------------------------------------------------------------------------------
def row_walk(addr, n, V, ld, itemsize):
    """(head, nvec, tail0) of row n as RowWalk in csrc/kvq_ce.hip splits it: scalar head up to the next 16-byte boundary,
    16-byte vectors, scalar tail from tail0.  addr = byte address of the view's first element."""
    vec = 16 // itemsize
    base = addr + n * ld * itemsize
    mis = base & 15
    head = (16 - mis) // itemsize if mis else 0
    head = min(head, V)
    nvec = (V - head) // vec
    return head, nvec, head + nvec * vec


def walk_positions(head, nvec, tail0, V, vec):
    """The distinct column positions at which a target or a maximum exercises another part of the walk."""
    pos = {0, V - 1}
    if head:
        pos.add(head - 1)
    if nvec:
        pos.update({head, head + vec - 1, head + (nvec - 1) * vec, tail0 - 1})
    if tail0 < V:
        pos.add(tail0)
    return sorted(p for p in pos if 0 <= p < V)


def ce_ref(x, target, c=1.0):
    """f64 reference from the up-cast logits x [N, V] (CPU): dict of lse, row_loss, pred (first arg-max), grad = c (softmax - onehot)."""
    x = x.detach().cpu().double()
    t = target.detach().cpu().long()
    lse = torch.logsumexp(x, dim=1)
    xt = x.gather(1, t[:, None])[:, 0]
    m = x.max(dim=1, keepdim=True).values
    V = x.shape[1]
    idx = torch.arange(V)[None, :].expand_as(x)
    pred = torch.where(x == m, idx, torch.full_like(idx, V)).min(dim=1).values        # FIRST index of the maximum
    p = torch.exp(x - lse[:, None])
    onehot = torch.zeros_like(x).scatter_(1, t[:, None], 1.0)
    return dict(lse=lse, row_loss=lse - xt, pred=pred, grad=float(c) * (p - onehot), cp=float(c) * p,
                absmax=x.abs().masked_fill(torch.isinf(x), 0).max(dim=1).values)


def ce_magnitude(ref):
    """M = max(1, |lse_ref|, max_j |x_j|) per row."""
    return torch.maximum(torch.maximum(torch.ones_like(ref["lse"]), ref["lse"].abs()), ref["absmax"])


def ce_row_ratio(got, ref_val, ref):
    """|got - ref| / (2^-20 M): eight f32 ulps at magnitude M."""
    return (got.detach().cpu().double() - ref_val).abs() / (2.0 ** -20 * ce_magnitude(ref))


def ce_large_row_slack(ref):
    """2^-20 M for the rows where that allowed lse error exceeds the gradient's rtol of 2e-5 (M > 21), else 0."""
    slack = 2.0 ** -20 * ce_magnitude(ref)
    return torch.where(slack > 2e-5, slack, torch.zeros_like(slack))


def ce_grad_ratio(got, ref, bf16, target):
    """Per-element |got - ref| over rtol 2e-5, atol 1e-8 (f32), plus one bf16 ulp 2^-8 |ref| for bf16 storage.

    The backward forms p = exp(x - lse) from the STORED f32 lse, which may be off by 2^-20 M: p then carries that relative
    error, an absolute c p 2^-20 M on the gradient.  Two places where rtol |ref| does not cover it get it on top:
      - the target's column, where ref = c (p - 1) cancels while the error of p does not (a dominant target: p ~ 1, ref ~ 0);
      - rows where 2^-20 M exceeds the rtol itself (M > 21: the rows shifted by 1e4, whose lse has an ulp of 1e-3).
    Every other element keeps the plain tolerance."""
    g = ref["grad"]
    lse_err = 2.0 ** -20 * ce_magnitude(ref)
    slack = ce_large_row_slack(ref)[:, None].expand_as(g).clone()
    t = target.detach().cpu().long()[:, None]
    slack.scatter_(1, t, lse_err[:, None])
    tol = 1e-8 + 2e-5 * g.abs() + (2.0 ** -8 * g.abs() if bf16 else 0.0) + slack * ref["cp"].abs()
    return (got.detach().cpu().double() - g).abs() / tol


def ce_tile_stats(x, V, tiles, tile=256):
    """stats [N][tiles][4] f32 as the LM-head GEMM's epilogue leaves them, built from the up-cast logits x [N, >=V] (CPU): per
    256-column tile (max, sum of exp(x - max) in f64 rounded to f32, first arg-max as int bits, 0) over the columns below V; a
    tile wholly beyond V, or whose maximum is -inf, carries sum 0 (and INT_MAX beyond V)."""
    x = x.detach().cpu().double()
    N = x.shape[0]
    st = torch.zeros(N, tiles, 4, dtype=torch.float32)
    ib = torch.zeros(N, tiles, dtype=torch.int32)
    for t in range(tiles):
        lo, hi = t * tile, min((t + 1) * tile, V)
        if lo >= hi:
            st[:, t, 0] = -math.inf
            ib[:, t] = INT_MAX
            continue
        seg = x[:, lo:hi]
        m = seg.max(dim=1).values
        s = torch.exp(seg - m[:, None]).sum(1)
        s = torch.where(torch.isinf(m), torch.zeros_like(s), s)
        st[:, t, 0] = m.float()
        st[:, t, 1] = s.float()
        ib[:, t] = (lo + (seg == m[:, None]).int().argmax(dim=1)).int()
    st[:, :, 2] = ib.view(torch.float32)
    return st
