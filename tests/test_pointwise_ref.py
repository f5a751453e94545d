"""CPU self-check of tests/_pointwise_ref.py: every judge accepts a plain f32 / bf16 torch restatement of the operation and
rejects each planted mistake on the output it hits.  Without this a judge that accepts everything would go unnoticed."""
import math

import pytest
import torch

import _pointwise_ref as R


# ---------------------------------------------------------------------------------------------------------------
# reductions
# ---------------------------------------------------------------------------------------------------------------
def _f32_sum_grouped(src, scale, dst0, out_dtype):
    """An f32 restatement with another grouping than index order (four interleaved partial sums, like the kernels)."""
    x = src.float()
    acc = [x[k::4].sum(0) for k in range(4)]
    a = ((acc[0] + acc[1]) + (acc[2] + acc[3])) * scale
    if dst0 is not None:
        a = a + dst0.to(out_dtype).float()
    return a.to(out_dtype)


REDUCE_MUTATIONS = {
    "drops its last row": lambda s: s[:-1],
    "doubles its first row": lambda s: torch.cat([s[:1], s]),
    "skips the remainder of a 4-unrolled loop": lambda s: s[:1 + 4 * ((s.shape[0] - 1) // 4)],
}


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("count,cols,scale,acc", [(1, 1, 1.0, False), (7, 13, 0.5, True), (4096, 8, -2.0, True), (33, 65, 1.0, True),
                                                  (130, 5, -2.0, False)])
def test_reduce_judge(count, cols, scale, acc, out_dtype):
    src = R.int_values((count, cols), count * 7 + cols)
    assert int(src.abs().min()) >= 1 and int(src.abs().max()) <= 8
    dst0 = R.int_values((cols,), 3) if acc else None
    ref = R.reduce_ref(src, scale, dst0)
    assert R.judge_exact(_f32_sum_grouped(src, scale, dst0, out_dtype), ref) == 0
    for name, mut in REDUCE_MUTATIONS.items():
        bad = mut(src)
        if bad.shape[0] == src.shape[0]:
            continue                                               # count - 1 is a multiple of 4: that loop has no remainder
        wrong = R.judge_exact(_f32_sum_grouped(bad, scale, dst0, out_dtype), ref)
        # one row of non-zero values: every f32 column is off (a bf16 destination can round a large sum to the same value: the
        # GPU tests run every case with an f32 destination too)
        one_row = abs(bad.shape[0] - count) == 1 and out_dtype == torch.float32
        assert wrong == cols if one_row else wrong > 0, f"a reduction that {name} was accepted"
    # the remainder mutation is hit by at least one of the cases above
    assert any(REDUCE_MUTATIONS["skips the remainder of a 4-unrolled loop"](torch.zeros(c, 1)).shape[0] != c for c in (7, 4096, 130))


def test_block_sums_judge():
    x = R.int_values((3 * 128 + 1, 13), 5)
    part = R.block_sums(x, 128)
    assert part.shape == (4, 13) and torch.equal(part[3], x[384].double())
    got = torch.stack([x[r:r + 128].float().sum(0) for r in range(0, 385, 128)])
    assert R.judge_exact(got, part) == 0
    got[1] -= x[255].float()                                       # block 1 drops its last row
    assert R.judge_exact(got, part) == 13


def test_integer_cases_stay_exact():
    """The largest case of the reduction tests: 4096 rows of +-8, scale -2, an integer destination of 8: far below 2^24."""
    worst = torch.full((4096, 4), 8, dtype=torch.int64)
    ref = R.reduce_ref(worst, -2.0, torch.full((4,), -8, dtype=torch.int64))
    assert float(ref.abs().max()) == 4096 * 8 * 2 + 8 < R.EXACT_LIMIT
    with pytest.raises(AssertionError):
        R.assert_exact_range(torch.tensor([float(1 << 23)]))
    with pytest.raises(AssertionError):
        R.assert_exact_range(torch.tensor([0.25]))
    # bf16 judge: a single RNE rounding; 257 lies halfway between 256 and 258 and goes to the even 256
    assert R.judge_exact(torch.tensor([256.0]).bfloat16(), torch.tensor([257.0])) == 0
    assert R.judge_exact(torch.tensor([258.0]).bfloat16(), torch.tensor([257.0])) == 1
    assert R.judge_exact(torch.tensor([-0.0]), torch.tensor([0.0])) == 0 and R.judge_exact(torch.tensor([-0.0]).bfloat16(), torch.tensor([0.0])) == 0


# ---------------------------------------------------------------------------------------------------------------
# GELU
# ---------------------------------------------------------------------------------------------------------------
def _as_f32(x):
    """The bf16 kernels' formula restated in f32 torch ops: (cdf, exp(-x^2/2))."""
    x = x.float()
    z = x.abs() * 0.70710678118654752
    t = 1.0 / (1.0 + 0.3275911 * z)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    e = torch.exp(-z * z)
    half_tail = 0.5 * poly * e
    return torch.where(x >= 0, 1.0 - half_tail, half_tail), e


def _erf_f32(x):
    x = x.float()
    cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752))
    return cdf, torch.exp(-0.5 * x * x)


def test_gelu_delta_is_measured():
    delta, worst, at = R.gelu_delta()
    assert delta == 2 * worst and 0.5e-7 < worst <= 0.75e-7 + 1e-9, (worst, at)       # A&S quote 1.5e-7 on erf = 0.75e-7 on the CDF


def test_gelu_bf16_judge():
    xs, fin = R.all_bf16_values()
    assert xs.numel() == 65536 and xs.numel() % 8 == 0 and int(fin.sum()) == 65536 - 2 * 128
    x = xs[fin]
    fwd, bwd = R.gelu_ref(x)
    cdf, e = _as_f32(x)
    xf = x.float()
    assert float(R.gelu_bf16_ratio((xf * cdf).bfloat16(), x, fwd, False).max()) <= 1.0
    assert float(R.gelu_bf16_ratio((cdf + xf * 0.39894228040143268 * e).bfloat16(), x, bwd, True).max()) <= 1.0
    assert float(R.gelu_bf16_ratio(cdf.bfloat16(), x, bwd, True).max()) > 1.0, "a GELU derivative without the x phi term was accepted"
    tanh = torch.nn.functional.gelu(xf, approximate="tanh")
    assert float(R.gelu_bf16_ratio(tanh.bfloat16(), x, fwd, False).max()) > 1.0, "a tanh-form GELU was accepted"
    assert float(R.gelu_bf16_ratio((-xf * cdf).bfloat16(), x, fwd, False).max()) > 1.0


def test_gelu_f32_judge():
    xs, fin = R.all_bf16_values()
    g = torch.Generator().manual_seed(1)
    x = torch.cat([xs[fin].float(), torch.rand(1 << 16, generator=g) * 24 - 12])
    fwd, bwd = R.gelu_ref(x)
    cdf, e = _erf_f32(x)
    assert float(R.f32_ratio(x * cdf, fwd).max()) <= 1.0
    assert float(R.f32_ratio(cdf + x * 0.39894228040143268 * e, bwd).max()) <= 1.0
    assert float(R.f32_ratio(cdf, bwd).max()) > 1.0, "a GELU derivative without the x phi term was accepted"
    assert float(R.f32_ratio(torch.nn.functional.gelu(x, approximate="tanh"), fwd).max()) > 1.0, "a tanh-form GELU was accepted"


def test_gelu_grad_is_exact_at_plus_minus_16():
    """What the exact gelu_bwd_bias test rests on: in f32, in both code paths, gelu'(16) == 1 and gelu'(-16) == 0 exactly (the
    tail terms exp(-128) underflow to zero), so g * gelu'(h) is g or 0."""
    x = torch.tensor([16.0, -16.0])
    for parts, k in ((_as_f32, 0.39894228040143268), (_erf_f32, 0.39894228040143268)):
        cdf, e = parts(x)
        d = cdf + x * k * e
        assert d.dtype == torch.float32 and d.tolist() == [1.0, 0.0] and e.tolist() == [0.0, 0.0]
    assert math.exp(-128.0) < 2.0 ** -149                               # below the smallest f32 subnormal
    assert x.bfloat16().float().tolist() == [16.0, -16.0]


# ---------------------------------------------------------------------------------------------------------------
# reconstruction loss
# ---------------------------------------------------------------------------------------------------------------
def _ce_f32(x, t, c):
    x = x.float()
    m = x.max(dim=1, keepdim=True).values
    lse = (m + torch.log(torch.exp(x - m).sum(1, keepdim=True)))[:, 0]
    g = c * (torch.exp(x - lse[:, None]) - torch.nn.functional.one_hot(t, x.shape[1]).float())
    return lse, lse - x.gather(1, t[:, None])[:, 0], torch.argmax(x, dim=1), g


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_ce_judges(dtype):
    g = torch.Generator().manual_seed(2)
    N, V, c = 9, 1027, 1.7 / 9
    x = (4 * torch.randn(N, V, generator=g)).to(dtype)
    x[:, 5] = x.float().max() + 1
    x[:, 900] = x[:, 5]                                               # two equal maxima: the first one counts
    x[3, 17] = -math.inf
    t = torch.randint(0, V - 1, (N,), generator=g)
    ref = R.ce_ref(x.float(), t, c)
    assert torch.all(ref["pred"] == 5) and torch.all(torch.isfinite(ref["lse"])) and ref["grad"][3, 17] == 0
    bf = dtype == torch.bfloat16
    lse, rl, pred, grad = _ce_f32(x, t, c)
    grad = grad.to(dtype)
    assert float(R.ce_row_ratio(lse, ref["lse"], ref).max()) <= 1 and float(R.ce_row_ratio(rl, ref["row_loss"], ref).max()) <= 1
    assert torch.equal(pred, ref["pred"]) and float(R.ce_grad_ratio(grad, ref, bf, t).max()) <= 1
    last = V - 1 - torch.argmax(x.float().flip(1), dim=1)
    assert not torch.equal(last, ref["pred"]), "an arg-max that returns the last maximum was accepted"
    shifted = _ce_f32(x, t + 1, c)[3].to(dtype)
    assert float(R.ce_grad_ratio(shifted, ref, bf, t).min(dim=1).values.max()) <= 1      # most columns are untouched ...
    assert torch.all(R.ce_grad_ratio(shifted, ref, bf, t).max(dim=1).values > 1e3), "a gradient with its -1 one column to the right was accepted"
    xm = x.float().clone()
    xm[:, 5] = -math.inf                                              # lse without one (large) element
    assert torch.all(R.ce_row_ratio(_ce_f32(xm, t, c)[0], ref["lse"], ref) > 1), "an lse that omits one element was accepted"


def test_ce_small_omission_is_seen():
    """An omitted element of ordinary size moves the lse by about 1/V: far beyond 2^-20 at the sizes the GPU tests use."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 13, generator=g)
    t = torch.zeros(4, dtype=torch.long)
    ref = R.ce_ref(x, t)
    for j in range(13):
        xm = x.clone()
        xm[:, j] = -math.inf
        assert torch.all(R.ce_row_ratio(_ce_f32(xm, t, 1.0)[0], ref["lse"], ref) > 1)


def test_row_walk_and_positions():
    # f32 rows of V = 13 at ld = 13 from a 16-byte aligned base plus one element: misalignment cycles 4, 8, 12, 0 bytes
    heads = [R.row_walk(4096 + 4, n, 13, 13, 4)[0] for n in range(4)]
    assert heads == [3, 2, 1, 0]
    assert R.row_walk(4096, 0, 13, 13, 4) == (0, 3, 12) and R.row_walk(4096 + 2, 0, 13, 13, 2) == (7, 0, 7)
    assert R.row_walk(4096 + 2, 0, 3, 3, 2) == (3, 0, 3)                       # the head is cut at V
    assert R.walk_positions(3, 2, 11, 13, 4) == [0, 2, 3, 6, 7, 10, 11, 12]
    assert R.walk_positions(0, 0, 0, 1, 8) == [0]


def test_tile_stats():
    x = torch.tensor([[0.0, 1.0, 1.0] + [-math.inf] * 253 + [-math.inf] * 256 + [1.0, 0.5]])
    st = R.ce_tile_stats(x, 514, 4)
    bits = st[0, :, 2].contiguous().view(torch.int32).tolist()
    assert st[0, :, 0].tolist() == [1.0, -math.inf, 1.0, -math.inf] and bits == [1, 256, 512, R.INT_MAX]
    assert st[0, 1, 1] == 0 and st[0, 3, 1] == 0 and abs(float(st[0, 0, 1]) - (2 + math.exp(-1))) < 1e-6
