"""CPU self-check of tests/_gemm_ref.py: every judge accepts a plain torch f32 restatement of the GEMM kernels' contract (f32
accumulation, bias added in f32, one RNE rounding; the accumulate chain rounds twice; GELU / GELU' of the stored bf16 values)
and rejects each planted mistake.  Without this a judge that accepts everything would go unnoticed."""
import math

import pytest
import torch

import _gemm_ref as G
import _pointwise_ref as R

BF16 = torch.bfloat16
M, N = 264, 200                    # not a multiple of any tile; more than one 16 x 16 block and one 64-deep k-tile everywhere
KS = (64, 128, 192, 256, 448)


def _trunc_bf16(v):
    """f32 -> bf16 by dropping the low 16 bits (the planted store without rounding)."""
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


def _restate(c, mistake=None):
    """The contract in plain f32 torch (another summation order than any kernel's: exact all the same), with one planted mistake."""
    A, B = c.A.float(), c.B.float()
    K = c.K
    if mistake == "dropped k-tile":
        A = A.clone()
        A[:, K - 64:] = 0
    acc = A @ B
    if mistake == "k-tile added twice":
        acc = acc + A[:, :64] @ B[:64]
    bias = c.bias.float() if c.bias is not None else None
    if mistake == "bias shifted by 4 columns":
        bias = bias.roll(4)
    store = _trunc_bf16 if mistake == "truncating store" else (lambda v: v.to(BF16))
    if mistake == "bias after rounding":
        r = store(store(acc).float() + bias)
    else:
        r = store(acc + bias if bias is not None else acc)
    if c.c_old is not None:
        if mistake == "single rounding in the accumulate chain":
            r = store((acc + bias if bias is not None else acc) + c.c_old.float())
        else:
            r = store(r.float() + c.c_old.float())
    return _output_mistake(r, mistake)


def _output_mistake(r, mistake):
    if mistake == "transposed 16x16 block":
        r = r.clone()
        r[16:32, 32:48] = r[16:32, 32:48].t().clone()
    if mistake == "row taken from row M-1":
        r = r.clone()
        r[r.shape[0] - 9] = r[r.shape[0] - 1]
    return r


GEMM_MISTAKES = ["truncating store", "dropped k-tile", "k-tile added twice", "transposed 16x16 block", "row taken from row M-1"]
BIAS_MISTAKES = ["bias after rounding", "bias shifted by 4 columns"]


@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("K", KS)
def test_exact_judge_accepts_the_contract_and_rejects_mistakes(layout, K):
    for bias, accumulate in ((False, False), (True, False), (True, True)):
        c = G.make_case(layout, M, N, K, seed=K + 7, bias=bias, accumulate=accumulate, padded=(K == 192))
        top, q = G.case_exact_range(c)
        assert q == 1.0 and top <= 64 * K + 8 + 8 * 32
        y, final, want = G.case_ref(c)
        assert G.exact_report(_restate(c), final) == (0, [])
        assert torch.equal(R.bf16_bits(_restate(c)), R.bf16_bits(want))
        mistakes = GEMM_MISTAKES + (BIAS_MISTAKES if bias else []) + (["single rounding in the accumulate chain"] if accumulate else [])
        for m in mistakes:
            bad, first = G.exact_report(_restate(c, m), final)
            assert bad > 0 and len(first) == min(bad, 5), f"{layout} K={K}: a kernel with '{m}' was accepted"
            r0, k0, got, wanted = first[0]
            assert got != wanted
            if m in ("dropped k-tile", "k-tile added twice"):
                assert bad > 0.5 * M * N, (m, bad)                    # a whole k-tile of non-zero integers moves most elements
            if m == "row taken from row M-1":
                assert all(r == M - 9 for r, *_ in first)
            if m == "transposed 16x16 block":
                assert all(16 <= r < 32 and 32 <= k < 48 for r, k, *_ in first)


def test_cases_discriminate_between_rounding_rules():
    """The plain cases need rounding on a good share of their elements and hold exact ties (y an odd multiple of half an ulp), so
    truncation, round-half-up and round-half-away are all told from RNE."""
    for K in KS:
        c = G.make_case("nt", M, N, K, seed=K + 7)
        y, final, want = G.case_ref(c)
        assert float(y.abs().max()) < 4096
        inexact = want.double() != y
        tie = (want.double() - y).abs() * 2 == _ulp(y)
        assert inexact.float().mean() > 0.08 and int(tie.sum()) > 1000, (K, float(inexact.float().mean()), int(tie.sum()))
        # ties rounded away from zero instead of to even
        away = torch.where(tie, y + torch.sign(y) * _ulp(y) / 2, y).float().to(BF16)
        assert R.judge_exact(away, final) > 0.25 * int(tie.sum())


def _ulp(y):
    """The bf16 spacing at |y| (f64)."""
    e = torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -126)))
    return 2.0 ** (e - 7)


def test_layouts_and_padded_parents():
    for layout in G.LAYOUTS:
        c = G.make_case(layout, 72, 40, 64, seed=3, bias=True, accumulate=True, padded=True)
        want_a = (64, 72) if layout == "tn" else (72, 64)
        want_b = (40, 64) if layout == "nt" else (64, 40)
        assert tuple(c.a.shape) == want_a and tuple(c.b.shape) == want_b
        for t in (c.a, c.b):
            assert t.stride() == (t.shape[1] + G.PAD_LD, 1) and t.storage_offset() == G.PAD_OFF and t.dtype == BF16
            base = t._base
            assert torch.isnan(base[:, :G.PAD_OFF].float()).all() and torch.isnan(base[:, G.PAD_OFF + t.shape[1]:].float()).all()
            assert torch.isfinite(t.float()).all()
        d = G.make_case(layout, 72, 40, 64, seed=3, bias=True, accumulate=True)
        assert d.a.is_contiguous() and torch.equal(d.a, c.a) and torch.equal(d.b, c.b) and torch.equal(d.A, c.A)
        assert torch.equal(G.on_device(c.a, "cpu"), c.a) and G.on_device(c.a, "cpu").stride() == c.a.stride()
        assert int(c.A.abs().min()) >= 1 and int(c.A.abs().max()) <= 8 and int(c.c_old.float().abs().max()) <= 8 * 32


def test_range_assertion_fires():
    # 2^24 reached by the sum of magnitudes although the result is small: 2^19 products of 7 * 7 with alternating signs
    K = 1 << 19
    A = torch.full((1, K), 7.0, dtype=torch.float64)
    B = torch.full((K, 1), 7.0, dtype=torch.float64)
    B[1::2] = -7.0
    assert float((A @ B).abs().max()) == 0
    with pytest.raises(AssertionError, match="exact f32 range"):
        G.assert_gemm_exact_range(A, B)
    G.assert_gemm_exact_range(A[:, :K // 2], B[:K // 2])
    # operands scaled by powers of two stay exact; a bias or an old C off the products' quantum does not
    c = G.make_case("nn", 16, 24, 64, seed=1, bias=True, accumulate=True, ea=-3, eb=-2)
    top, q = G.case_exact_range(c)
    assert q == 2.0 ** -5
    with pytest.raises(AssertionError, match="quantum"):
        G.assert_gemm_exact_range(c.A, c.B, c.bias.double() + 2.0 ** -6)
    with pytest.raises(AssertionError, match="quantum"):
        G.assert_gemm_exact_range(c.A, c.B, None, c.c_old.double() * 0.5)
    with pytest.raises(AssertionError, match="exact f32 range"):
        G.assert_gemm_exact_range(c.A, c.B, torch.full((24,), 2.0 ** 19, dtype=torch.float64))
    assert G.quantum(torch.tensor([6.0, -0.75, 0.0])) == 0.25


# ---------------------------------------------------------------------------------------------------------------
# fused epilogues
# ---------------------------------------------------------------------------------------------------------------
def _as_gelu_f32(h):
    """GELU and GELU' of bf16 h the way the kernels compute them: the A&S erf in f32 (tests/_pointwise_ref.py: as_cdf_f64)."""
    x = h.float()
    cdf, e = R.as_cdf_f64(x)
    cdf, e = cdf.float(), e.float()
    return x * cdf, cdf + x * R.INV_SQRT_2PI * e


def _gelu_case():
    c0 = G.make_case("nt", M, N, 192, seed=21, bias=True)
    e = G.pick_exponent(G.case_ref(c0)[0], 6.0)
    c = G.make_case("nt", M, N, 192, seed=21, bias=True, ea=e // 2, eb=e - e // 2, ebias=e + 5)
    G.case_exact_range(c)
    return c


def test_gelu_epilogue_judge():
    c = _gelu_case()
    y, final, want = G.case_ref(c)
    assert 4.0 <= float(y.abs().max()) <= 9.0 and float(y.std()) > 1.0
    h = _restate(c)
    a = _as_gelu_f32(h)[0].to(BF16)
    assert G.exact_report(h, final)[0] == 0
    assert float(G.gelu_epilogue_ratio(a, h).max()) <= 1.0
    # mistakes of the product show in Hout (exact judge); the activation of a wrong Hout is still that Hout's activation
    for m in GEMM_MISTAKES + BIAS_MISTAKES:
        hb = _restate(c, m)
        assert G.exact_report(hb, final)[0] > 0, m
    # mistakes of the second output show in the GELU judge, against the h that was stored
    planted = {
        "truncating store": _trunc_bf16(_as_gelu_f32(h)[0]),
        "transposed 16x16 block": _output_mistake(a, "transposed 16x16 block"),
        "row taken from row M-1": _output_mistake(a, "row taken from row M-1"),
        "activation of the unrounded sum": _as_gelu_f32((c.A.float() @ c.B.float() + c.bias.float()))[0].to(BF16),
        "tanh form": torch.nn.functional.gelu(h.float(), approximate="tanh").to(BF16),
    }
    for name, bad in planted.items():
        over = int((G.gelu_epilogue_ratio(bad, h) > 1.0).sum())
        assert over > 0, f"a GELU epilogue with '{name}' was accepted"


def test_dgelu_epilogue_judge():
    c = G.make_case("nn", M, N, 128, seed=31)
    G.case_exact_range(c)
    y, final, g = G.case_ref(c)
    h = G.all_h_values(M, N, seed=32)
    xs, fin = R.all_bf16_values()
    need = xs[fin & (xs.float().abs() <= 8)]
    assert set(R.bf16_bits(need).tolist()) <= set(R.bf16_bits(h).reshape(-1).tolist()) and float(h.float().abs().max()) == 8.0
    d = _as_gelu_f32(h)[1]
    out = (g.float() * d).to(BF16)
    assert float(G.dgelu_epilogue_ratio(out, g, h).max()) <= 1.0
    planted = {m: (_restate(c, m).float() * d).to(BF16) for m in GEMM_MISTAKES}
    planted["truncating store"] = _trunc_bf16(g.float() * d)                                  # of the output itself
    planted["truncating store of the product"] = (_trunc_bf16(c.A.float() @ c.B.float()).float() * d).to(BF16)
    planted["derivative of the unrounded product"] = ((c.A.float() @ c.B.float()) * d).to(BF16)
    planted["h taken one column over"] = (g.float() * _as_gelu_f32(h.roll(1, dims=1))[1]).to(BF16)
    planted["gelu instead of gelu'"] = (g.float() * _as_gelu_f32(h)[0]).to(BF16)
    for name, bad in planted.items():
        over = int((G.dgelu_epilogue_ratio(bad, g, h) > 1.0).sum())
        assert over > 0, f"a GELU' epilogue with '{name}' was accepted"
    # the bias-gradient partials: f32 sums of the stored values in another grouping pass; a row tile that drops its last row does not
    for bm in (128, 256):
        tiles = -(-M // bm)
        part = torch.stack([sum(out[t * bm:(t + 1) * bm][k::4].float().sum(0) for k in range(4)) for t in range(tiles)])
        assert G.dgelu_part_check(part, out, bm) <= 1.0
        short = part.clone()
        short[0] -= out[bm - 1].float()
        assert G.dgelu_part_check(short, out, bm) > 1.0
        with pytest.raises(AssertionError):
            G.dgelu_part_check(part[:-1], out, bm)


def test_ce_stats_judge():
    V, NP, K = 510, 520, 64
    c0 = G.make_case("nt", 40, NP, K, seed=41, bias=True)
    e = G.pick_exponent(G.case_ref(c0)[0], 8.0)
    c = G.make_case("nt", 40, NP, K, seed=41, bias=True, ea=e // 2, eb=e - e // 2, ebias=e + 5)
    c.bias[V:] = 50.0
    G.case_exact_range(c)
    logits = G.case_ref(c)[2]
    logits[:, 128:256] = logits[:, :128]                                     # every maximum of the first tile's first half is tied
    tiles = (NP + 255) // 256
    assert tiles == 3 and 2 * 256 >= V                                       # the last tile lies wholly beyond V
    x = logits.float()
    st = torch.zeros(40, tiles, 4)
    ib = torch.zeros(40, tiles, dtype=torch.int32)
    for t in range(tiles):
        seg = x[:, t * 256:min((t + 1) * 256, V)]
        if seg.shape[1] == 0:
            st[:, t, 0], ib[:, t] = -math.inf, R.INT_MAX
            continue
        m = seg.max(dim=1).values
        st[:, t, 0] = m
        st[:, t, 1] = torch.exp(seg - m[:, None]).sum(1)                   # f32
        ib[:, t] = t * 256 + (seg == m[:, None]).int().argmax(dim=1).int()
    st[:, :, 2] = ib.view(torch.float32)
    res = G.ce_stats_judge(st, logits, V)
    assert (res["max_bad"], res["arg_bad"], res["pad_bad"]) == (0, 0, 0) and float(res["ratio"].max()) <= 1.0
    assert res["ratio"].shape == (40, 2)
    # tied maxima: the LAST arg-max instead of the first is caught
    last = st.clone()
    lb = ib.clone()
    seg = x[:, :256]
    lb[:, 0] = (255 - (seg.flip(1) == seg.max(dim=1, keepdim=True).values).int().argmax(dim=1)).int()
    assert int((lb[:, 0] != ib[:, 0]).sum()) > 0, "no tied maximum in the case"
    last[:, :, 2] = lb.view(torch.float32)
    assert G.ce_stats_judge(last, logits, V)["arg_bad"] == int((lb[:, 0] != ib[:, 0]).sum())
    # the padding columns (bias 50) counted; the sum without its maximum's own term; a padded tile left at zero
    pad = st.clone()
    pad[:, 1, 0] = x[:, 256:512].max(dim=1).values
    assert G.ce_stats_judge(pad, logits, V)["max_bad"] == 40
    short = st.clone()
    short[:, 0, 1] -= 1.0
    assert float(G.ce_stats_judge(short, logits, V)["ratio"][:, 0].min()) > 1.0
    zero = st.clone()
    zero[:, 2] = 0
    assert G.ce_stats_judge(zero, logits, V)["pad_bad"] == 40
