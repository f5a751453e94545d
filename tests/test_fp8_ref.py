"""CPU self-check of tests/_fp8_ref.py: the decode tables equal torch's float8 types on all 256 bytes, quant_ref equals torch's
clamp -> conversion on all 65536 bf16 patterns under every scale the GPU tests use, and each GEMM judge accepts a plain torch f32
restatement of the fp8 kernels' contract (f32 accumulation of the decoded operands, mul = 1 / (sa sb) in f32, bias added in f32, one
RNE rounding; the accumulate chain rounds twice) and rejects each planted mistake.  Run with -s for the counts
(profiles/fp8_exact_parity.md)."""
import math

import pytest
import torch

import _fp8_ref as F8
import _gemm_ref as G
import _pointwise_ref as R

BF16 = torch.bfloat16
M, N = 136, 264                    # the GPU file's smallest two-tile shape: not a multiple of any tile, several 16 x 16 blocks
KS = (128, 384, 896)
QUANT_SCALES = (1.0, 37.5, 2.0 ** -6, 2.0 ** 12, 448.0 / 2.0 ** 20, 57344.0 / 2.0 ** 20, 448.0 / 786432.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------
# formats and quantisation
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", F8.FORMATS)
def test_decode_equals_torch_on_all_bytes(fmt):
    b = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    mine, theirs = F8.decode(b, fmt), b.view(F8.FMT_TORCH[fmt]).double()
    assert torch.equal(torch.isnan(mine), torch.isnan(theirs))
    ok = ~torch.isnan(mine)
    assert torch.equal(mine[ok], theirs[ok]) and torch.equal(torch.signbit(mine[ok]), torch.signbit(theirs[ok]))
    nan = [i for i in range(256) if math.isnan(float(mine[i]))]
    inf = [i for i in range(256) if math.isinf(float(mine[i]))]
    if fmt == F8.E4M3:
        assert nan == [0x7F, 0xFF] and inf == [] and float(mine[0x7E]) == 448.0 and float(mine[1]) == 2.0 ** -9
    else:
        assert nan == [0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF] and inf == [0x7C, 0xFC] and float(mine[0x7B]) == 57344.0 and float(mine[1]) == 2.0 ** -16
    fin = torch.isfinite(mine)
    assert torch.equal(F8.encode_exact(mine[fin], fmt), b[fin])
    with pytest.raises(AssertionError):
        F8.encode_exact(torch.tensor([17.0]), fmt)                 # five significant bits


@pytest.mark.parametrize("scale", QUANT_SCALES)
@pytest.mark.parametrize("fmt", F8.FORMATS)
def test_quant_ref_equals_torch_on_all_bf16_patterns(fmt, scale):
    x, fin = R.all_bf16_values()
    s = torch.tensor(scale, dtype=torch.float32)
    fmax = F8.FMT_MAX[fmt]
    theirs = (x.float() * s).clamp(-fmax, fmax).to(F8.FMT_TORCH[fmt]).view(torch.uint8)
    mine = F8.quant_ref(x, s, fmt)
    bad, first = F8.quant_report(theirs, mine, fmt)
    assert bad == 0, (fmt, scale, bad, first)
    assert F8.quant_report(mine, theirs, fmt)[0] == 0
    val = F8.decode(mine, fmt)
    p = x.float() * s
    assert torch.equal(torch.isnan(val), torch.isnan(p))                               # a NaN stays one, nothing else becomes one
    assert bool(torch.isfinite(val[~torch.isnan(p)]).all())                            # +-inf saturates
    assert torch.equal(torch.signbit(val[~torch.isnan(p)]), torch.signbit(p[~torch.isnan(p)]))   # -0 and underflow keep the sign
    if scale == 1.0:
        # exact ties go to the even code, the last value below saturation stays below, subnormals are there
        assert F8.quant_ref(torch.tensor([17.0, 19.0, 2.0 ** -10, 3 * 2.0 ** -10]).to(BF16), 1.0, F8.E4M3).tolist() == \
            F8.encode_exact(torch.tensor([16.0, 20.0, 0.0, 2.0 ** -8]), F8.E4M3).tolist()
        assert F8.quant_ref(torch.tensor([464.0, 466.0, -1e9]).to(BF16), 1.0, F8.E4M3).tolist() == [0x7E, 0x7E, 0xFE]
        assert len(set(mine.tolist())) >= 2 * F8.N_FINITE[fmt]


def test_quant_report_rejects_wrong_bytes():
    x, fin = R.all_bf16_values()
    want = F8.quant_ref(x, 37.5, F8.E4M3)
    p = (x.float() * 37.5)
    trunc = p.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    assert F8.quant_report(trunc, want, F8.E4M3)[0] == 0
    planted = {
        "no clamp (saturation lost)": p.to(torch.float8_e4m3fn).view(torch.uint8),
        "the other format": p.clamp(-448, 448).to(torch.float8_e5m2).view(torch.uint8),
        "scale 37 instead of 37.5": F8.quant_ref(x, 37.0, F8.E4M3),
        "subnormals flushed": torch.where(F8.decode(want, F8.E4M3).abs() < 2.0 ** -6, want & 0x80, want),
        "NaN clamped to the maximum": torch.where(torch.isnan(p), torch.full_like(want, 0x7E), want),
        "sign of zero dropped": torch.where(F8.decode(want, F8.E4M3) == 0, torch.zeros_like(want), want),
        "ties away from zero (scale 1)": _ties_away(x.float(), F8.quant_ref(x, 1.0, F8.E4M3)),
    }
    for name, got in planted.items():
        bad = F8.quant_report(got, F8.quant_ref(x, 1.0, F8.E4M3) if "ties" in name else want, F8.E4M3)[0]
        print(f"FIGURE quant_report, '{name}': {bad} of 65536 patterns")
        assert bad > 0, f"a quantisation with '{name}' was accepted"
    assert F8.amax_ref(x) == math.inf and F8.amax_ref(x[fin]) == float(x[fin].float().abs().max()) and F8.amax_ref(x[:0]) == 0.0


def _ties_away(p, want):
    """want with every exact tie between two e4m3 codes moved to the code away from zero."""
    tab = F8.decode_table(F8.E4M3)
    code = (want & 0x7F).long().clamp_max(0x7E)
    mag = torch.nan_to_num(p.double().abs(), 0.0).clamp_max(448.0)
    lo = torch.where(tab[code] <= mag, code, code - 1).clamp_min(0)
    up = (lo + 1).clamp_max(0x7E)
    tie = ((mag - tab[lo]) == (tab[up] - mag)) & (up > lo) & ~torch.isnan(p)
    assert int(tie.sum()) > 100
    return torch.where(tie, (up | (want & 0x80).long()).to(torch.uint8), want)


# ---------------------------------------------------------------------------------------------------------------
# GEMM judges
# ---------------------------------------------------------------------------------------------------------------
def _trunc_bf16(v):
    """f32 -> bf16 by dropping the low 16 bits (the planted store without rounding)."""
    return (v.contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF16)


def _restate(c, mistake=None):
    """The contract in plain f32 torch from the BYTES of the case, with one planted mistake."""
    a8, b8 = c.a8.clone(), c.b8
    if mistake == "fragment halves swapped in A":
        a8 = a8.reshape(c.M, c.K // 32, 2, 16).flip(2).reshape(c.M, c.K)
    A = F8.decode(a8, F8.E4M3 if mistake == "A decoded as e4m3" else c.a_fmt).float()
    B = F8.decode(b8, F8.E4M3).float().t()
    if mistake == "dropped k-tile":
        A = A.clone()
        A[:, c.K - 128:] = 0
    acc = A @ B
    if mistake == "k-tile added twice":
        acc = acc + A[:, :128] @ B[:128]
    mul = 1.0 / c.sa if mistake == "mul from sa alone" else 1.0 / (c.sa * c.sb)            # f32
    bias = c.bias.float() if c.bias is not None else None
    if mistake == "bias shifted by 4 columns":
        bias = bias.roll(4)
    store = _trunc_bf16 if mistake == "truncating store" else (lambda v: v.to(BF16))
    if mistake == "bias after rounding":
        r = store(store(acc * mul).float() + bias)
    elif mistake == "scale applied to the bias":
        r = store((acc + bias) * mul)
    else:
        r = store(acc * mul + bias if bias is not None else acc * mul)
    if c.c_old is not None:
        if mistake == "single rounding in the accumulate chain":
            r = store((acc * mul + bias if bias is not None else acc * mul) + c.c_old.float())
        else:
            r = store(r.float() + c.c_old.float())
    if mistake == "transposed 16x16 block":
        r = r.clone()
        r[16:32, 32:48] = r[16:32, 32:48].t().clone()
    return r


GEMM_MISTAKES = ["truncating store", "mul from sa alone", "dropped k-tile", "k-tile added twice", "fragment halves swapped in A",
                 "transposed 16x16 block"]
BIAS_MISTAKES = ["bias after rounding", "scale applied to the bias", "bias shifted by 4 columns"]


def _mistakes(c):
    return GEMM_MISTAKES + (BIAS_MISTAKES if c.bias is not None else []) + (["A decoded as e4m3"] if c.a_fmt == F8.E5M2 else []) + \
        (["single rounding in the accumulate chain"] if c.c_old is not None else [])


@pytest.mark.parametrize("a_fmt", F8.FORMATS)
@pytest.mark.parametrize("K", KS)
def test_exact_judge_accepts_the_contract_and_rejects_mistakes(K, a_fmt):
    for bias, accumulate in ((False, False), (True, False), (True, True)):
        c = F8.make_case8(M, N, K, seed=K + 7, a_fmt=a_fmt, bias=bias, accumulate=accumulate, padded=(K == 384))
        top, q = F8.case8_exact_range(c)
        assert q == 1.0 and top <= 64 * K + 2 * (8 + 8 * 32) and c.mul == 0.5
        y, final, want = F8.case8_ref(c)
        assert G.exact_report(_restate(c), final) == (0, [])
        assert torch.equal(R.bf16_bits(_restate(c)), R.bf16_bits(want))
        for m in _mistakes(c):
            bad, first = G.exact_report(_restate(c, m), final)
            print(f"FIGURE exact judge K={K} {a_fmt} bias={bias} accumulate={accumulate}, '{m}': {bad} of {M * N}")
            assert bad > 0 and len(first) == min(bad, 5), f"K={K} {a_fmt}: a kernel with '{m}' was accepted"
            if m in ("dropped k-tile", "k-tile added twice", "fragment halves swapped in A", "mul from sa alone", "A decoded as e4m3"):
                assert bad > 0.5 * M * N, (m, bad)
            if m == "transposed 16x16 block":
                assert all(16 <= r < 32 and 32 <= k < 48 for r, k, *_ in first)


def _ulp(y):
    e = torch.floor(torch.log2(y.abs().clamp_min(2.0 ** -126)))
    return 2.0 ** (e - 7)


def test_cases_discriminate_between_rounding_rules():
    """The plain cases need rounding on a good share of their elements and hold exact ties."""
    for K in KS:
        c = F8.make_case8(M, N, K, seed=K + 7)
        y, final, want = F8.case8_ref(c)
        inexact = want.double() != y
        tie = (want.double() - y).abs() * 2 == _ulp(y)
        caught = G.exact_report(_restate(c, "truncating store"), final)[0]
        print(f"FIGURE K={K}: max|y| {float(y.abs().max()):.0f}, {float(inexact.double().mean()):.1%} of the outputs need rounding, "
              f"{int(tie.sum())} exact ties, truncating store caught on {caught} of {M * N}")
        assert inexact.float().mean() > 0.08 and int(tie.sum()) > 1000
        away = torch.where(tie, y + torch.sign(y) * _ulp(y) / 2, y).float().to(BF16)
        assert R.judge_exact(away, final) > 0.25 * int(tie.sum())


@pytest.mark.parametrize("a_fmt", F8.FORMATS)
@pytest.mark.parametrize("K", KS)
def test_interval_judge_accepts_the_contract_and_rejects_mistakes(K, a_fmt):
    c = F8.make_case8(M, N, K, seed=K + 9, a_fmt=a_fmt, bias=True, sa=448.0 / 37.3, sb=448.0 / 1.9)
    assert not c.exact
    F8.case8_exact_range(c)
    lo, hi, share = F8.interval_ref(c)
    print(f"FIGURE interval judge K={K} {a_fmt}: {share:.4%} of the elements have two admissible values")
    assert F8.interval_report(_restate(c), lo, hi) == (0, [])
    # the same contract with the multiplications in another order stays inside as well: (acc / sa) / sb
    A, B = F8.decode(c.a8, c.a_fmt).float(), F8.decode(c.b8, F8.E4M3).float().t()
    other = (((A @ B) / c.sa) / c.sb + c.bias.float()).to(BF16)
    assert F8.interval_report(other, lo, hi)[0] == 0
    for m in _mistakes(c):
        bad, first = F8.interval_report(_restate(c, m), lo, hi)
        print(f"FIGURE interval judge K={K} {a_fmt}, '{m}': {bad} of {M * N}")
        assert bad > 0 and len(first) == min(bad, 5), f"K={K} {a_fmt}: a kernel with '{m}' was accepted"
    nan = _restate(c).clone()
    nan[3, 5] = float("nan")
    assert F8.interval_report(nan, lo, hi)[0] == 1
    with pytest.raises(AssertionError, match="two admissible"):
        F8.interval_ref(c, max_two_valued=-1.0)


def test_rne_bf16_f64_rounds_once():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -(1.0 + 2.0 ** -8 - 2.0 ** -40), 0.0, 255.5, 3.0e-5],
                     dtype=torch.float64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.0, 256.0, 3.0e-5], dtype=torch.float64)
    got = F8.rne_bf16_f64(x)
    assert torch.equal(got[:7].double(), want[:7]) and got[7] == torch.tensor(3.0e-5).to(BF16)
    # through f32 the fourth value would be rounded twice: 1 + 2^-8 + 2^-40 -> (f32) 1 + 2^-8 -> (tie to even) 1
    assert float(x[3].float().to(BF16)) == 1.0


def test_padded_parents_and_the_range_assertion():
    c = F8.make_case8(72, 40, 128, seed=3, a_fmt=F8.E5M2, bias=True, accumulate=True, padded=True, ea=-2, eb=1)
    for t in (c.a8, c.b8):
        assert t.stride() == (128 + F8.PAD8_LD, 1) and t.storage_offset() == F8.PAD8_OFF and t.dtype == torch.uint8
        base = t._base
        assert bool((base[:, :F8.PAD8_OFF] == 0x7F).all()) and bool((base[:, F8.PAD8_OFF + 128:] == 0x7F).all())
    for fmt in F8.FORMATS:
        assert math.isnan(float(F8.decode_table(fmt)[F8.NAN_BYTE]))
    d = F8.make_case8(72, 40, 128, seed=3, a_fmt=F8.E5M2, bias=True, accumulate=True, ea=-2, eb=1)
    assert torch.equal(d.a8, c.a8) and torch.equal(d.b8, c.b8) and d.a8.is_contiguous()
    top, q = F8.case8_exact_range(c)
    assert q == 0.5 and c.q == 0.5 and float(c.bias.double().abs().min()) >= q * c.mul
    u = F8.make_case8(72, 40, 128, seed=3, unit=True)
    assert F8.case8_exact_range(u)[0] == 128 and float(u.A.abs().max()) == 1.0
    # K = 2048 with full operands passes 2^17 quanta although it is exact in f32: refused
    big = F8.make_case8(8, 8, 2048, seed=1)
    G.assert_gemm_exact_range(big.A, big.B)
    if float((big.A.abs() @ big.B.abs()).max()) >= F8.ACC_LIMIT:
        with pytest.raises(AssertionError, match="2\\^17"):
            F8.case8_exact_range(big)
    with pytest.raises(AssertionError):
        F8.make_case8(8, 8, 128, seed=1, ea=6)                     # 8 * 2^6 is beyond e4m3
    with pytest.raises(AssertionError):
        F8.make_case8(8, 8, 128, seed=1, accumulate=True, sa=3.0)  # an old C needs the exact judge


@pytest.mark.parametrize("fmt,slot", [(F8.E4M3, "a"), (F8.E5M2, "a"), (F8.E4M3, "b")])
def test_one_hot_cases(fmt, slot):
    c, want = F8.one_hot_case(fmt, slot)
    tab = F8.decode_table(fmt)
    sw = c.a8 if slot == "a" else c.b8
    assert sorted(sw[sw != 0].tolist()) == list(range(1, 256)) and int((sw != 0).sum(1).max()) == 1
    w = want if slot == "a" else want.t()                           # [pattern, other row]
    assert torch.equal(torch.isnan(w), torch.isnan(tab)[:, None].expand_as(w))
    assert torch.equal(torch.isinf(w), torch.isinf(tab)[:, None].expand_as(w))
    assert len(set((w[1] / tab[1]).tolist())) == 5                  # five different powers of two meet each pattern
    # a plain f32 matmul of the decoded operands gives these values wherever no NaN / inf byte takes part ...
    fin = torch.isfinite(tab)
    A, B = c.A.clone(), c.B.clone()
    out = ((torch.nan_to_num(A, 0.0, 0.0, 0.0).float() @ torch.nan_to_num(B, 0.0, 0.0, 0.0).float()) * 0.5).to(BF16)
    rows = fin if slot == "a" else torch.ones(c.M, dtype=torch.bool)
    cols = fin if slot == "b" else torch.ones(c.N, dtype=torch.bool)
    sub = lambda t: t[rows][:, cols]
    assert F8.one_hot_report(sub(out), sub(want)) == (0, [])
    # ... a finite value where a NaN or an inf is due is caught, and so is the pattern decoded in the other format
    assert F8.one_hot_report(out, want)[0] == int((~fin).sum()) * F8.ONE_HOT_OTHER
    wrong = F8.E5M2 if fmt == F8.E4M3 else F8.E4M3
    c2, want2 = F8.one_hot_case(wrong, "a") if slot == "a" else (None, None)
    if c2 is not None:
        bad = F8.one_hot_report(sub(want2.float().to(BF16)), sub(want))[0]
        print(f"FIGURE one-hot {fmt} {slot}: the other format's decoding differs on {bad} of {int(rows.sum()) * int(cols.sum())} finite outputs")
        assert bad > 200 * F8.ONE_HOT_OTHER


# ---------------------------------------------------------------------------------------------------------------
# the tile query (no launch: answers on a host without a GPU, where the library assumes 256 CUs)
# ---------------------------------------------------------------------------------------------------------------
def test_tile_query_restates_the_rule():
    import os
    import re
    from kvq import _ffi
    lib = _ffi.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8 if torch.cuda.is_available() else 256
    env = re.match(r"\s*[+-]?\d+", os.environ.get("KVQ_FP8_TILE", "1"))
    narrow_ok = not ("KVQ_FP8_TILE" in os.environ and (int(env.group()) if env else 0) == 0)
    assert lib.kvq_gemm_fp8_tile(0, 8) == -1 and lib.kvq_gemm_fp8_tile(8, 0) == -1
    for m in (8, 136, 264, 8192, 32768, 65536):
        for n in (8, 200, 264, 392, 520, 768, 1352, 1800, 3072):
            tm = -(-m // 128)
            t256, t192 = tm * -(-n // 256), tm * -(-n // 192)
            want = _ffi.GEMM_TILE_128x192 if narrow_ok and t256 < cus and t192 > t256 else _ffi.GEMM_TILE_128x256
            assert lib.kvq_gemm_fp8_tile(m, n) == want, (m, n)
