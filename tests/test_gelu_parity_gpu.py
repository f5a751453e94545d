"""Per-element parity of the GELU kernels (gelu_kernel, gelu_tail_kernel, gelu_bwd_bias_kernel of csrc/kvq_nn.hip) against f64.

bf16: all 65536 bit patterns, judged inside  2^-8 |ref| + delta |x| + 2^-126  (forward) and  2^-8 |ref| + delta (1 + |x|) + 2^-126
(backward): one bf16 ulp of output rounding plus the absolute error of the Abramowitz-Stegun erf the bf16 kernels use; delta is
twice that formula's own worst error on the CDF, measured in f64 (tests/_pointwise_ref.py: gelu_delta).  f32: rtol = atol = 1e-5.
gelu_bwd_bias: exact on h = +-16 (gelu' is exactly 1 or 0 there) and integer g, at row counts that reach the remainder loop and
row blocks of fewer than 4 rows.  Measured figures: profiles/pointwise_parity.md."""
import itertools

import pytest
import torch

import _pointwise_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = 77.0
PAD = 64


@pytest.fixture(scope="module")
def ops():
    from kvq import _ffi, nnops
    _ffi.lib()
    assert torch.cuda.is_available()
    return nnops


@pytest.fixture(scope="module")
def sweep():
    """The inputs and their f64 references, computed once: all bf16 patterns (finite ones judged), and for f32 those values
    plus 2^16 random ones in [-12, 12]."""
    xs, fin = R.all_bf16_values()
    g = torch.Generator().manual_seed(11)
    x32 = torch.cat([torch.where(fin, xs.float(), torch.zeros(())), torch.rand(1 << 16, generator=g) * 24 - 12])
    d = dict(xb=xs, fin=fin, x32=x32)
    d["fwd_b"], d["bwd_b"] = R.gelu_ref(xs.float()[fin])
    d["fwd_f"], d["bwd_f"] = R.gelu_ref(x32)
    return d


def _report(name, ratio, x):
    i = int(ratio.argmax())
    print(f"FIGURE {name}: worst ratio {float(ratio[i]):.4f} at x = {float(x[i]):.8g}")
    return float(ratio[i])


def test_gelu_bf16_all_patterns(ops, sweep):
    xb, fin = sweep["xb"], sweep["fin"]
    assert xb.numel() % 8 == 0
    h = xb.cuda()
    a = ops.gelu_fwd(h).cpu()[fin]
    gh = ops.gelu_bwd(h, torch.ones_like(h)).cpu()[fin]
    x = xb[fin].double()
    delta, worst, at = R.gelu_delta()
    print(f"FIGURE gelu delta = {delta:.6e} (A&S formula in f64: worst CDF error {worst:.6e} at x = {at:.6g})")
    rf = R.gelu_bf16_ratio(a, x, sweep["fwd_b"], False)
    rb = R.gelu_bf16_ratio(gh, x, sweep["bwd_b"], True)
    wf, wb = _report("gelu bf16 fwd", rf, x), _report("gelu bf16 bwd", rb, x)
    # where the approximation stops being below the bf16 rounding of the result: relative error of the stored forward value
    ref = sweep["fwd_b"]
    nz = ref.abs() >= 2.0 ** -126
    rel = torch.where(nz, (a.double() - ref).abs() / ref.abs().clamp_min(2.0 ** -126), torch.zeros_like(ref))
    i = int(rel.argmax())
    print(f"FIGURE gelu bf16 fwd largest relative error {float(rel[i]):.4g} at x = {float(x[i]):.8g}")
    # RNE rounding alone reaches 2^-9 relative at any magnitude and stays below 2^-8: beyond 2^-8 the approximation shows
    for name, lim in (("2^-9", 2.0 ** -9), ("2^-8", 2.0 ** -8)):
        over = nz & (rel > lim)
        if bool(over.any()):
            print(f"FIGURE gelu bf16 fwd relative error exceeds {name} at {int(over.sum())} values, the largest x = {float(x[over].max()):.8g}; "
                  f"all negative: {bool((x[over] < 0).all())}")
    # sign and monotone step at the x >= 0 switch
    assert torch.all(a.float()[x > 0] >= 0) and torch.all(a.float()[x < 0] <= 0), "gelu has the sign of x"
    assert torch.all(a.float()[x == 0] == 0)
    assert wf <= 1.0 and wb <= 1.0, (wf, wb)


def test_gelu_bf16_monotone_at_the_switch(ops, sweep):
    """cdf switches formula at x >= 0: the derivative must step up through 0.5 without a dip, and the forward through 0."""
    xb, fin = sweep["xb"], sweep["fin"]
    h = xb.cuda()
    gh = ops.gelu_bwd(h, torch.ones_like(h)).cpu().float()
    a = ops.gelu_fwd(h).cpu().float()
    x = xb.float()
    sel = fin & (x.abs() <= 2.0 ** -6)
    order = torch.argsort(x[sel], stable=True)
    assert torch.all(gh[sel][order].diff() >= 0), "gelu' is not monotone through x = 0"
    small = fin & (x.abs() <= 0.5)                                     # gelu itself rises from its minimum at x = -0.7518 on
    order = torch.argsort(x[small], stable=True)
    assert torch.all(a[small][order].diff() >= 0), "gelu is not monotone through x = 0"
    assert float(gh[(x == 0) & fin].min()) == 0.5 == float(gh[(x == 0) & fin].max())


def test_gelu_f32_sweep(ops, sweep):
    h = sweep["x32"].cuda()
    assert h.numel() % 8 == 0
    a = ops.gelu_fwd(h)
    gh = ops.gelu_bwd(h, torch.ones_like(h))
    wf = _report("gelu f32 fwd (rtol=atol=1e-5)", R.f32_ratio(a, sweep["fwd_f"]), sweep["x32"])
    wb = _report("gelu f32 bwd (rtol=atol=1e-5)", R.f32_ratio(gh, sweep["bwd_f"]), sweep["x32"])
    assert wf <= 1.0 and wb <= 1.0, (wf, wb)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gelu_sizes(ops, sweep, dtype):
    """The 8-chunk body alone, the 4-element tail alone and after a body, and the grid stride; a sentinel follows the output."""
    from kvq._ffi import check, io_dtype_of, lib, stream_ptr
    src = sweep["x32"][65536:] if dtype == F32 else sweep["xb"].float()[sweep["fin"]][torch.randperm(65280, generator=torch.Generator().manual_seed(5))]
    for n in (4, 8, 12, 2044, 2048, 2052, 256 * 8 * 3 + 4):
        x = src[:n].to(dtype)
        fwd, bwd = R.gelu_ref(x.float())
        g = R.int_values((n,), n).to(dtype)
        h = x.cuda()
        for backward in (False, True):
            out = torch.full((n + PAD,), SENTINEL, dtype=dtype, device="cuda")
            if backward:
                check(lib().kvq_gelu_bwd(h.data_ptr(), g.cuda().data_ptr(), out.data_ptr(), n, io_dtype_of(h), stream_ptr()), "gelu_bwd")
                ref, scale = bwd * g.double(), g.double().abs()
            else:
                check(lib().kvq_gelu_fwd(h.data_ptr(), out.data_ptr(), n, io_dtype_of(h), stream_ptr()), "gelu_fwd")
                ref, scale = fwd, torch.ones(n, dtype=torch.float64)
            assert torch.all(out[n:] == SENTINEL), f"n={n}: wrote past the output"
            got = out[:n].cpu()
            if dtype == F32:
                ratio = R.f32_ratio(got, ref, 1e-5, 1e-5) if not backward else (got.double() - ref).abs() / (scale * (1e-5 + 1e-5 * (ref / scale).abs()))
            else:
                # g is an integer of at most 4 bits: g * gelu'(x) carries gelu's own envelope times |g|
                d = R.gelu_delta()[0]
                xd = x.double()
                env = ref.abs() * 2.0 ** -8 + scale * d * ((1 + xd.abs()) if backward else xd.abs()) + R.TINY
                ratio = (got.double() - ref).abs() / env
            assert float(ratio.max()) <= 1.0, f"n={n} {dtype} backward={backward}: ratio {float(ratio.max()):.3f} at element {int(ratio.argmax())}"


GB_ROWS = 8


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gelu_bwd_bias_exact(ops, dtype):
    """h in {+16, -16}, integer g: g_h is g or 0 exactly, every partial row the integer column sum of its 8-row block.  N walks
    the 4-row body, the one-row remainder loop and row blocks of fewer than 4 rows."""
    from kvq._ffi import check, io_dtype_of, lib, stream_ptr
    for N, C in itertools.product((1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13, 16 + 6), (8, 1016, 1024, 1032, 2048 + 8)):
        gi = R.int_values((N, C), N * 131 + C)
        sign = R.int_values((N, C), N * 137 + C + 1) > 0
        h = torch.where(sign, 16.0, -16.0).to(dtype).cuda()
        g = gi.to(dtype).cuda()
        P = lib().kvq_gelu_bwd_partial_rows(N)
        assert P == (N + GB_ROWS - 1) // GB_ROWS
        gh = torch.full((N * C + 2 * PAD,), SENTINEL, dtype=dtype, device="cuda")
        part = torch.full((P * C + 2 * PAD,), SENTINEL, dtype=F32, device="cuda")
        check(lib().kvq_gelu_bwd_bias(h.data_ptr(), g.data_ptr(), gh[PAD:].data_ptr(), N, C, io_dtype_of(h), part[PAD:].data_ptr(), P * C * 4,
                                      stream_ptr()), "gelu_bwd_bias")
        what = f"gelu_bwd_bias N={N} C={C} {dtype}"
        for buf, n in ((gh, N * C), (part, P * C)):
            assert torch.all(buf[:PAD] == SENTINEL) and torch.all(buf[PAD + n:] == SENTINEL), f"{what}: wrote outside its output"
        want = torch.where(sign, gi, torch.zeros_like(gi))
        assert torch.equal(gh[PAD:PAD + N * C].view(N, C).cpu().double(), want.double()), f"{what}: g_h is not g or 0"
        ref_part = R.block_sums(want, GB_ROWS)
        got = part[PAD:PAD + P * C].view(P, C).cpu()
        wrong = [p for p in range(P) if R.judge_exact(got[p], ref_part[p])]
        assert not wrong, f"{what}: partial rows {wrong} differ from the exact block sums"


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gelu_bwd_bias_real_values(ops, dtype):
    """N = 13, C = 1032: g_h bit-identical to gelu_bwd, each partial row the f32 sum of the stored values of its block: at most 7
    f32 additions of partial sums bounded by the column's sum of |g_h|, half an ulp each, relative 2^-24."""
    torch.manual_seed(13)
    N, C = 13, 1032
    h = (3 * torch.randn(N, C)).to(dtype).cuda()
    g = torch.randn(N, C).to(dtype).cuda()
    gh, part = ops.gelu_bwd_bias(h, g)
    assert torch.equal(gh, ops.gelu_bwd(h, g)) and part.shape == (2, C)
    st = gh.cpu().double()
    for p in range(2):
        blk = st[p * GB_ROWS:(p + 1) * GB_ROWS]
        bound = 7 * 2.0 ** -24 * blk.abs().sum(0)
        err = (part[p].cpu().double() - blk.sum(0)).abs()
        assert torch.all(err <= bound), f"partial row {p}: worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}"
