"""Bit-exact parity of the fp8 GEMMs (gemm2_f8_kernel of csrc/kvq_gemm2.hip through kvq_gemm_fp8_nt, kvq_gemm_fp8_nt_ex and
kvq_gemm_fp8_nt_gelu) against an f64 matmul of the decoded operands on the CPU, and of the quantisation passes (csrc/kvq_fp8.hip;
quant8 / quant8_fmt / amax8 of csrc/kvq_common.h) against quant_ref on every bf16 pattern.  References, cases and judges:
tests/_fp8_ref.py (checked on the CPU by tests/test_fp8_ref.py).

GEMM operands are integers in [-8, 8] without 0 times a power of two, exact in e4m3 and e5m2, with S = |A| . |B| below 2^17 quanta
(case8_exact_range, before every launch); with power-of-two scales the stored value must be bf16_rne(A . B / (sa sb) + bias) bit for
bit -- with accumulate bf16_rne(bf16_rne(.) + C_old); with other scales it must lie in the interval of _fp8_ref.interval_ref.  Every
output sits in a canary frame (bf16 CANARY for C / Hout / Aout, 0xAB for bytes) whose bits must not change; padded operands sit in
parents of NaN bytes.  Every GEMM test asserts the tile arm (kvq_gemm_fp8_tile) it names:
  k-tiles 1, 2, 3, 4, 7 against the ring of 3 and the body written out twice: test_core K = 128 .. 896, on both arms
  9 tiles (ntiles % 8 != 0): test_core 264 x 520 x 256;  8 tile columns, band of 6 and a narrower last band: 136 x 1352 x 128 (128x192)
  bias clamp, accumulate chain, lda / ldb / ldc != widths and a 16-byte offset: test_variants
  every byte pattern of either operand, one product per output: test_single_products
Every test judges every element.  Measured figures and the arm-by-arm list of test ids: profiles/fp8_exact_parity.md."""
import functools
import math
import os
import re

import pytest
import torch

import _fp8_ref as F8
import _gemm_ref as G
import _pointwise_ref as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
CANARY = 77.0
BYTE_CANARY = 0xAB
WIDE, NARROW = "128x256", "128x192"
_TILE_ENV = re.match(r"\s*[+-]?\d+", os.environ.get("KVQ_FP8_TILE", "1"))
NARROW_OFF = "KVQ_FP8_TILE" in os.environ and (int(_TILE_ENV.group()) if _TILE_ENV else 0) == 0      # the library's atoi(...) == 0
ENTRIES = ("nt", "ex-e4m3", "ex-e5m2")             # kvq_gemm_fp8_nt; kvq_gemm_fp8_nt_ex with A in e4m3 / e5m2
SA, SB = 8.0, 0.25                                 # power-of-two device scales: mul = 1/2


@pytest.fixture(scope="module")
def ops():
    from kvq import _ffi, nnops
    _ffi.lib()
    assert torch.cuda.is_available()
    return nnops


def _arm(ops, M, N, want):
    """Skip the narrow-arm tests under KVQ_FP8_TILE=0; assert that the launch of an [M, N] output takes the tile the test names."""
    if want == NARROW and NARROW_OFF:
        pytest.skip("KVQ_FP8_TILE=0: the fp8 GEMMs always take the 128x256 tile")
    got = ops.gemm_fp8_tile(M, N)
    assert got == want, f"[{M}, {N}] runs on the {got} tile, the test is meant for {want}"


def _fmt_of(entry):
    return F8.E5M2 if entry == "ex-e5m2" else F8.E4M3


@functools.lru_cache(maxsize=None)
def _case(M, N, K, seed, a_fmt, bias=False, accumulate=False, padded=False, ea=0, eb=0):
    """A power-of-two-scale case, checked to be inside the exact range, and the f64 value whose RNE rounding must be stored."""
    c = F8.make_case8(M, N, K, seed, a_fmt=a_fmt, bias=bias, accumulate=accumulate, padded=padded, ea=ea, eb=eb, sa=SA, sb=SB)
    F8.case8_exact_range(c)
    return c, F8.case8_ref(c)[1]


def _framed(M, N, c_old=None):
    frame = torch.full((M + 2, N + 16), CANARY, dtype=BF16, device="cuda")
    out = frame[1:M + 1, 8:8 + N]
    if c_old is not None:
        out.copy_(c_old)
    return frame, out


def _frame_intact(frame, M, N):
    f = frame.cpu().float()
    return bool((f[0] == CANARY).all() and (f[M + 1] == CANARY).all() and (f[:, :8] == CANARY).all() and (f[:, 8 + N:] == CANARY).all())


def _launch(ops, c, entry, what):
    """The case through one of the three entries into a canary frame (ldc = N + 16); the output on the CPU."""
    assert (entry == "ex-e5m2") == (c.a_fmt == F8.E5M2) and (entry != "nt" or c.c_old is None)
    a8, b8 = G.on_device(c.a8), G.on_device(c.b8)
    bias = c.bias.cuda() if c.bias is not None else None
    frame, out = _framed(c.M, c.N, c.c_old)
    ops.gemm_fp8_nt(a8, b8, c.sa.cuda().reshape(1), c.sb.cuda().reshape(1), bias=bias, out=out,
                    a_format=None if entry == "nt" else c.a_fmt, accumulate=c.c_old is not None)
    torch.cuda.synchronize()
    assert _frame_intact(frame, c.M, c.N), f"{what}: wrote outside its output"
    return out.cpu()


_OUTPUTS = {}


def _run(ops, entry, key, what):
    """One launch per (entry, case); test_entry_equivalence reads the outputs the other tests left (or makes them)."""
    if (entry, key) not in _OUTPUTS:
        _OUTPUTS[(entry, key)] = _launch(ops, _case(*key)[0], entry, what)
    return _OUTPUTS[(entry, key)]


# ---------------------------------------------------------------------------------------------------------------
# the tile rule
# ---------------------------------------------------------------------------------------------------------------
def test_tile_query(ops):
    """kvq_gemm_fp8_tile restated: 128x192 where 128x256 leaves CUs without a tile and 128x192 gives more tiles."""
    from kvq._ffi import lib
    assert lib().kvq_gemm_fp8_tile(0, 8) == -1 and lib().kvq_gemm_fp8_tile(8, -8) == -1
    cus = ops.cu_count(torch.device("cuda", 0)) // 8 * 8
    for M, N in [(8, 8), (136, 264), (136, 392), (136, 200), (264, 520), (136, 1352), (136, 1800), (8192, 768), (8192, 3072), (65536, 768)]:
        tm = -(-M // 128)
        t256, t192 = tm * -(-N // 256), tm * -(-N // 192)
        want = NARROW if (not NARROW_OFF and t256 < cus and t192 > t256) else WIDE
        assert ops.gemm_fp8_tile(M, N) == want, (M, N)
    if not NARROW_OFF and cus == 256:
        assert ops.gemm_fp8_tile(8192, 768) == NARROW and ops.gemm_fp8_tile(8192, 3072) == WIDE


# ---------------------------------------------------------------------------------------------------------------
# exact judge
# ---------------------------------------------------------------------------------------------------------------
KS = (128, 256, 384, 512, 896)                     # 1, 2, 3, 4, 7 k-tiles
CORE = [(WIDE, (8, 8, 128))] + [(WIDE, (136, 264, K)) for K in KS] + [(WIDE, (264, 520, 256))] + \
       [(NARROW, (136, 392, K)) for K in KS] + [(NARROW, (136, 1352, 128))]
CORE_IDS = [f"{t}-{m}x{n}x{k}" for t, (m, n, k) in CORE]


def _core_key(shape, entry):
    M, N, K = shape
    return (M, N, K, M + 3 * N + 5 * K, _fmt_of(entry))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("tile,shape", CORE, ids=CORE_IDS)
def test_core(ops, tile, shape, entry):
    M, N, K = shape
    _arm(ops, M, N, tile)
    key = _core_key(shape, entry)
    what = f"{entry} {tile} {shape}"
    G.assert_exact(_run(ops, entry, key, what), _case(*key)[1], what)


VARIANTS = {"bias": dict(bias=True), "accumulate": dict(accumulate=True), "strided": dict(padded=True),
            "all": dict(bias=True, accumulate=True, padded=True)}
VARIANT_CASES = [(t, v, e) for t in (WIDE, NARROW) for v in VARIANTS for e in ENTRIES if not (e == "nt" and "accumulate" in VARIANTS[v])]


def _variant_key(tile, variant, entry):
    M, N, K = 136, (256 if tile == WIDE else 192) + 8, 384       # N = BN + 8: the last 16-column block is half outside
    v = VARIANTS[variant]
    return (M, N, K, M + N + 11, _fmt_of(entry), v.get("bias", False), v.get("accumulate", False), v.get("padded", False))


@pytest.mark.parametrize("tile,variant,entry", VARIANT_CASES, ids=[f"{t}-{v}-{e}" for t, v, e in VARIANT_CASES])
def test_variants(ops, tile, variant, entry):
    key = _variant_key(tile, variant, entry)
    M, N, K = key[:3]
    _arm(ops, M, N, tile)
    c, final = _case(*key)
    if VARIANTS[variant].get("padded"):
        assert c.a8.stride(0) == K + F8.PAD8_LD and c.b8.stride(0) == K + F8.PAD8_LD and c.a8.storage_offset() == F8.PAD8_OFF
    what = f"{entry} {tile} {variant}"
    G.assert_exact(_run(ops, entry, key, what), final, what)


EQUIV = [_core_key(s, "nt") for _, s in CORE] + [_variant_key(t, v, "nt") for t in (WIDE, NARROW) for v in ("bias", "strided")]


@pytest.mark.parametrize("key", EQUIV, ids=[f"{k[0]}x{k[1]}x{k[2]}" + ("-bias" if len(k) > 5 and k[5] else "") + ("-strided" if len(k) > 7 and k[7] else "")
                                            for k in EQUIV])
def test_entry_equivalence(ops, key):
    """kvq_gemm_fp8_nt_ex(e4m3, accumulate = 0) stores the bits of kvq_gemm_fp8_nt, on the exact cases."""
    old, new = _run(ops, "nt", key, "nt"), _run(ops, "ex-e4m3", key, "ex-e4m3")
    assert torch.equal(R.bf16_bits(old), R.bf16_bits(new))


@pytest.mark.parametrize("fmt,slot", [(F8.E4M3, "a"), (F8.E5M2, "a"), (F8.E4M3, "b")])
def test_single_products(ops, fmt, slot):
    """Every byte pattern of an operand, each met by one power of two: the stored value is decode(byte) 2^e / (sa sb), whatever
    the adder does; NaN bytes give NaN, e5m2 inf bytes give +-inf."""
    c, want = F8.one_hot_case(fmt, slot)
    assert ops.gemm_fp8_tile(c.M, c.N) == (WIDE if slot == "a" or NARROW_OFF else NARROW)      # [256, 72] and [72, 256]
    entries = ("nt", "ex-e4m3") if fmt == F8.E4M3 else ("ex-e5m2",)
    for entry in entries:
        out = _launch(ops, c, entry, f"single products {fmt} {slot} {entry}")
        bad, first = F8.one_hot_report(out, want)
        assert bad == 0, f"single products, {fmt} patterns in {slot} through {entry}: {bad} wrong; first (row, col, got, want): {first}"


# ---------------------------------------------------------------------------------------------------------------
# interval judge: quantisation-style scales
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a_fmt", F8.FORMATS)
@pytest.mark.parametrize("tile", [WIDE, NARROW])
def test_interval(ops, tile, a_fmt):
    """The same operands under sa = 448 / 37.3, sb = 448 / 1.9 (f32; no powers of two) with a bias: the stored value lies between
    the roundings of v -+ (2^-22 |acc / (sa sb)| + 2^-24 |v|)."""
    M, N, K = 136, 264 if tile == WIDE else 392, 384
    _arm(ops, M, N, tile)
    c = F8.make_case8(M, N, K, seed=M + N + 17, a_fmt=a_fmt, bias=True, sa=448.0 / 37.3, sb=448.0 / 1.9)
    assert not c.exact
    F8.case8_exact_range(c)
    lo, hi, share = F8.interval_ref(c)
    print(f"FIGURE interval judge {tile} {a_fmt}: {share:.4%} of the elements have two admissible values")
    for entry in (("nt", "ex-e4m3") if a_fmt == F8.E4M3 else ("ex-e5m2",)):
        F8.assert_interval(_launch(ops, c, entry, f"interval {tile} {entry}"), lo, hi, f"interval {tile} {entry}")


# ---------------------------------------------------------------------------------------------------------------
# kvq_gemm_fp8_nt_gelu
# ---------------------------------------------------------------------------------------------------------------
def _state(scale, sites=1):
    from kvq._ffi import lib
    st = torch.zeros((sites, lib().kvq_fp8_state_floats()), dtype=torch.float32, device="cuda")
    st[:, 0] = scale
    return st


def _byte_frame(rows, ld, pad=64):
    """(buffer, view): rows x ld bytes inside a flat buffer of 0xAB with `pad` bytes before and after."""
    buf = torch.full((pad + rows * ld + pad,), BYTE_CANARY, dtype=torch.uint8, device="cuda")
    return buf, buf[pad:pad + rows * ld].view(rows, ld)


@pytest.mark.parametrize("shape", [(136, 264, 384), (136, 1800, 128)], ids=["136x264x384", "136x1800x128"])
def test_gelu_entry(ops, shape):
    """Hout exact; Aout = gelu(stored Hout) inside the bf16 forward envelope per element; the fp8 copy (row stride N + 8, inside a
    byte frame) = quant_ref(stored Aout, state[0], e4m3) and the noted amax = max |Aout|; the call without the copy stores the same
    Hout / Aout bits.  (136, 1800): eight tile columns, a band of six and a narrower last band."""
    from kvq._ffi import check, lib, stream_ptr
    M, N, K = shape
    c0, y0 = _case(M, N, K, 500 + N, F8.E4M3, True)
    e = G.pick_exponent(y0, 6.0)
    c, final = _case(M, N, K, 500 + N, F8.E4M3, True, False, False, e // 2, e - e // 2)
    assert 4.0 <= float(final.abs().max()) <= 9.0 and float(final.std()) > 0.9, "h does not spread over about +-6"
    a8, b8, bias = c.a8.cuda(), c.b8.cuda(), c.bias.cuda()
    sa, sb = c.sa.cuda().reshape(1), c.sb.cuda().reshape(1)
    scale8 = 120.0                                                  # max gelu(h) is between 4 and 9: the largest values saturate at 448
    runs = {}
    for copy in (True, False):
        hf, h = _framed(M, N)
        af, a = _framed(M, N)
        st = _state(scale8)
        buf8, a8out = _byte_frame(M, N + 8)
        check(lib().kvq_gemm_fp8_nt_gelu(a8.data_ptr(), b8.data_ptr(), sa.data_ptr(), sb.data_ptr(), bias.data_ptr(), h.data_ptr(), a.data_ptr(),
                                         a8out.data_ptr() if copy else None, N + 8 if copy else 0, st.data_ptr() if copy else None,
                                         M, N, K, K, K, h.stride(0), stream_ptr()), "kvq_gemm_fp8_nt_gelu")
        torch.cuda.synchronize()
        assert _frame_intact(hf, M, N) and _frame_intact(af, M, N), f"gelu entry {shape} copy={copy}: wrote outside its outputs"
        runs[copy] = (h.cpu(), a.cpu(), a8out.cpu(), buf8.cpu(), st.cpu())
    h, a, a8o, buf8, st = runs[True]
    G.assert_exact(h, final, f"gelu entry {shape}: Hout")
    ratio = G.gelu_epilogue_ratio(a, h)
    i = int(ratio.argmax())
    print(f"FIGURE fp8 gemm gelu epilogue {shape} (2^{e}): worst ratio {float(ratio.reshape(-1)[i]):.4f} at {divmod(i, N)}")
    assert float(ratio.max()) <= 1.0, f"{int((ratio > 1.0).sum())} elements of Aout outside the envelope"
    want8 = F8.quant_ref(a, scale8, F8.E4M3)
    bad, first = F8.quant_report(a8o[:, :N], want8, F8.E4M3)
    assert bad == 0, f"gelu entry {shape}: {bad} bytes of the fp8 copy differ; first (index, got, want): {first}"
    assert int((F8.decode(want8, F8.E4M3).abs() == 448.0).sum()) > 0, "no value of the copy saturates"
    assert bool((a8o[:, N:] == BYTE_CANARY).all()) and bool((buf8[:64] == BYTE_CANARY).all()) and bool((buf8[-64:] == BYTE_CANARY).all())
    assert float(st[0, 8:].max()) == F8.amax_ref(a) and float(st[0, 0]) == scale8
    h2, a2, a8o2, buf82, st2 = runs[False]
    assert torch.equal(R.bf16_bits(h2), R.bf16_bits(h)) and torch.equal(R.bf16_bits(a2), R.bf16_bits(a))
    assert bool((buf82 == BYTE_CANARY).all()) and float(st2[0, 8:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------
# quantisation passes on every bf16 pattern
# ---------------------------------------------------------------------------------------------------------------
SCALES = (1.0, 37.5, 2.0 ** -6, 2.0 ** 12)
VIEWS = {"dense": (512, 512), "strided": (512, 528), "narrow": (504, 520)}      # cols, row stride; 504 % 16 != 0: 8 elements per thread


@functools.lru_cache(maxsize=None)
def _patterns(kind):
    """bf16 [128, 512]: all 65536 patterns, shuffled ("all"); the same with inf and NaN replaced by 1 ("finite"); with everything
    beyond `kind` (a number) in magnitude, inf and NaN replaced by 1."""
    x, fin = R.all_bf16_values()
    if kind != "all":
        keep = fin if kind == "finite" else fin & (x.float().abs() <= float(kind))
        x = torch.where(keep, x, torch.ones_like(x))
    g = torch.Generator().manual_seed(65536)
    return x[torch.randperm(65536, generator=g)].reshape(128, 512).contiguous()


def _view(x, cols, ld, fill=float("nan")):
    """x[:, :cols] as a device view with row stride ld (the parent's other columns hold `fill`)."""
    parent = torch.full((x.shape[0], ld), fill, dtype=BF16)
    parent[:, :cols] = x[:, :cols]
    return parent.cuda()[:, :cols]


@functools.lru_cache(maxsize=None)
def _want_bytes(kind, cols, scale, fmt):
    return F8.quant_ref(_patterns(kind)[:, :cols], scale, fmt)


def _delayed(x, st, entry, out):
    """entry: "plain" = kvq_fp8_quantize_delayed (e4m3); "e4m3" / "e5m2" = kvq_fp8_quantize_delayed_fmt.  out None: amax only."""
    from kvq._ffi import check, lib, stream_ptr
    from kvq import nnops
    rows, cols = x.shape
    if entry == "plain":
        check(lib().kvq_fp8_quantize_delayed(x.data_ptr(), rows, cols, x.stride(0), out.data_ptr(), st.data_ptr(), stream_ptr()), "delayed")
    else:
        check(lib().kvq_fp8_quantize_delayed_fmt(x.data_ptr(), rows, cols, x.stride(0), None if out is None else out.data_ptr(), st.data_ptr(),
                                                 nnops.FP8_FORMATS[entry], stream_ptr()), "delayed_fmt")


@pytest.mark.parametrize("view", list(VIEWS))
@pytest.mark.parametrize("entry", ["plain", "e4m3", "e5m2"])
def test_delayed_passes_on_every_pattern(ops, entry, view):
    """Every bf16 pattern (and the finite ones alone) under scales 1, 37.5, 2^-6 (e4m3 subnormals and zero) and 2^12 (most values
    saturate): the bytes of quant_ref inside an untouched byte frame, the noted amax = max |x| over the non-NaN elements exactly
    (inf with the infinities in), the scale untouched; the amax-only form notes the same and writes nothing."""
    cols, ld = VIEWS[view]
    fmt = F8.E4M3 if entry == "plain" else entry
    for kind in ("all", "finite"):
        x = _view(_patterns(kind), cols, ld)
        assert x.stride(0) == ld and (cols % 16 == 0) == (view != "narrow")
        amax = F8.amax_ref(_patterns(kind)[:, :cols])
        assert math.isinf(amax) == (kind == "all")
        for scale in SCALES:
            st = _state(scale)
            buf, out = _byte_frame(128, cols)
            _delayed(x, st, entry, out)
            torch.cuda.synchronize()
            what = f"delayed {entry} {view} {kind} scale {scale}"
            bad, first = F8.quant_report(out.cpu(), _want_bytes(kind, cols, scale, fmt), fmt)
            assert bad == 0, f"{what}: {bad} bytes differ; first (index, got, want): {first}"
            b = buf.cpu()
            assert bool((b[:64] == BYTE_CANARY).all()) and bool((b[-64:] == BYTE_CANARY).all()), f"{what}: wrote outside its output"
            s = st.cpu()
            assert float(s[0, 8:].max()) == amax and float(s[0, 0]) == scale and float(s[0, 1:8].abs().max()) == 0.0, what
        if entry != "plain":
            st = _state(37.5)
            _delayed(x, st, entry, None)
            assert float(st.cpu()[0, 8:].max()) == amax and float(st.cpu()[0, 0]) == 37.5


def _self_scaling(x, fmt_arg):
    """kvq_fp8_quantize (fmt_arg None) / kvq_fp8_quantize_fmt: (bytes on the CPU, frame intact, amax, scale)."""
    from kvq._ffi import check, lib, stream_ptr
    from kvq import nnops
    rows, cols = x.shape
    buf, out = _byte_frame(rows, cols)
    st = torch.full((2,), -1.0, dtype=torch.float32, device="cuda")
    if fmt_arg is None:
        check(lib().kvq_fp8_quantize(x.data_ptr(), rows, cols, x.stride(0), out.data_ptr(), st[0:].data_ptr(), st[1:].data_ptr(), stream_ptr()), "quantize")
    else:
        check(lib().kvq_fp8_quantize_fmt(x.data_ptr(), rows, cols, x.stride(0), out.data_ptr(), st[0:].data_ptr(), st[1:].data_ptr(),
                                         nnops.FP8_FORMATS[fmt_arg], stream_ptr()), "quantize_fmt")
    torch.cuda.synchronize()
    b = buf.cpu()
    return out.cpu(), bool((b[:64] == BYTE_CANARY).all() and (b[-64:] == BYTE_CANARY).all()), float(st[0]), st[1].cpu()


SELF_ENTRIES = [(None, F8.E4M3), ("e4m3", F8.E4M3), ("e5m2", F8.E5M2)]


@pytest.mark.parametrize("view", list(VIEWS))
@pytest.mark.parametrize("fmt_arg,fmt", SELF_ENTRIES, ids=["plain", "e4m3", "e5m2"])
def test_self_scaling_passes_on_the_finite_patterns(ops, fmt_arg, fmt, view):
    """kvq_fp8_quantize[_fmt] on the finite patterns of |x| <= 2^20 (amax 2^20), and of |x| <= 3 * 2^18 (an amax whose quotient is
    inexact: IEEE division rounds it once): amax exact, scale == f32(max(fmt)) / amax in f32 exactly, the bytes of quant_ref under
    that scale."""
    cols, ld = VIEWS[view]
    for bound in (2.0 ** 20, 3 * 2.0 ** 18):
        x = _view(_patterns(bound), cols, ld, fill=2.0 ** 30)       # a read outside the view would raise the amax
        got, intact, amax, scale = _self_scaling(x, fmt_arg)
        what = f"self-scaling {fmt_arg} {view} bound {bound}"
        assert intact, f"{what}: wrote outside its output"
        assert amax == bound == F8.amax_ref(_patterns(bound)[:, :cols]), what
        want_scale = torch.tensor(F8.FMT_MAX[fmt], dtype=torch.float32) / torch.tensor(amax, dtype=torch.float32)
        assert torch.equal(scale, want_scale), f"{what}: scale {float(scale)!r}, wanted {float(want_scale)!r}"
        bad, first = F8.quant_report(got, F8.quant_ref(_patterns(bound)[:, :cols], scale, fmt), fmt)
        assert bad == 0, f"{what}: {bad} bytes differ; first (index, got, want): {first}"


@pytest.mark.parametrize("fmt_arg,fmt", SELF_ENTRIES, ids=["plain", "e4m3", "e5m2"])
def test_self_scaling_with_an_inf(ops, fmt_arg, fmt):
    """Pinned: one +inf makes the amax inf and the scale max(fmt) / inf = 0 -- every finite value becomes a (signed) zero, the inf
    itself 0 * inf = NaN; a NaN stays a NaN and does not enter the amax.  (The delayed passes saturate an inf instead: their scale
    does not come from this tensor.)"""
    x = _patterns(2.0 ** 20).clone()
    x[5, 17], x[77, 300] = float("inf"), float("nan")
    got, intact, amax, scale = _self_scaling(x.cuda(), fmt_arg)
    assert intact and math.isinf(amax) and float(scale) == 0.0
    val = F8.decode(got, fmt)
    assert math.isnan(float(val[5, 17])) and math.isnan(float(val[77, 300])) and int(torch.isnan(val).sum()) == 2
    rest = torch.ones_like(val, dtype=torch.bool)
    rest[5, 17] = rest[77, 300] = False
    assert bool((val[rest] == 0).all()) and torch.equal(torch.signbit(val[rest]), torch.signbit(x.float()[rest]))
    assert F8.quant_report(got, F8.quant_ref(x, scale, fmt), fmt)[0] == 0


# ---------------------------------------------------------------------------------------------------------------
# a planted maximum where an amax pass could lose it
# ---------------------------------------------------------------------------------------------------------------
PLANT_ROWS, PLANT_COLS, PLANT_LD = 1040, 1032, 1056     # 134160 chunks of 8: more than the 512 * 256 one trip of the delayed grid covers
PLANT_WIDE_COLS, PLANT_WIDE_LD = 2064, 2080             # 134160 chunks of 16: the second trip of the 16-per-thread arm


@functools.lru_cache(maxsize=None)
def _small_values(cols):
    g = torch.Generator().manual_seed(cols)
    return (torch.rand((PLANT_ROWS, cols), generator=g) * 2 - 1).to(BF16)


def _plant_positions(cols, per):
    """(name, row, col) of the places a maximum hides: first and last element, last chunk of the first row, first chunk of the last
    row, and chunk 512 * 256 + 1000 of `per` elements, which the delayed grid reaches on its second trip only."""
    cpr = cols // per
    c2 = 512 * 256 + 1000
    assert c2 < PLANT_ROWS * cpr
    return [("first element", 0, 0), ("last element", PLANT_ROWS - 1, cols - 1), ("last chunk of the first row", 0, cols - 3),
            ("first chunk of the last row", PLANT_ROWS - 1, 2), ("second grid-stride trip", c2 // cpr, (c2 % cpr) * per + per - 1)]


@pytest.mark.parametrize("layout", ["dense", "strided"])
@pytest.mark.parametrize("cols", [PLANT_COLS, PLANT_WIDE_COLS], ids=["8-per-thread", "16-per-thread"])
def test_planted_maximum_is_found(ops, cols, layout):
    """|x| <= 1 with one element of 100 (sign alternating); the strided view's parent holds 1000 beside the rows.  Every entry that
    produces an amax must report exactly 100: the delayed passes (both entries, both formats, amax-only) in the record's
    partials, the self-scaling passes in amax and as scale = max(fmt) / 100."""
    ld = cols if layout == "dense" else (PLANT_LD if cols == PLANT_COLS else PLANT_WIDE_LD)
    per = 16 if cols % 16 == 0 else 8
    base = _small_values(cols)
    out = torch.empty((PLANT_ROWS, cols), dtype=torch.uint8, device="cuda")
    for k, (name, r, col) in enumerate(_plant_positions(cols, per)):
        x = base.clone()
        x[r, col] = 100.0 if k % 2 == 0 else -100.0
        xd = _view(x, cols, ld, fill=1000.0)
        for entry in ("plain", "e4m3", "e5m2"):
            for amax_only in ((False, True) if entry != "plain" else (False,)):
                st = _state(1.0)
                _delayed(xd, st, entry, None if amax_only else out)
                assert float(st[0, 8:].max()) == 100.0, f"delayed {entry} amax_only={amax_only} {layout}: maximum at the {name} lost"
        for fmt_arg, fmt in SELF_ENTRIES:
            _, intact, amax, scale = _self_scaling(xd, fmt_arg)
            assert intact and amax == 100.0, f"self-scaling {fmt_arg} {layout}: maximum at the {name} lost ({amax})"
            assert torch.equal(scale, torch.tensor(F8.FMT_MAX[fmt], dtype=torch.float32) / torch.tensor(100.0, dtype=torch.float32))


@pytest.mark.parametrize("where", ["last 8", "first 8"])
@pytest.mark.parametrize("periodic", [False, True], ids=["segments", "periodic"])
def test_segment_maxima_stay_in_their_segments(ops, periodic, where):
    """kvq_fp8_quantize_segments[_periodic on a refresh step]: three segments of 8 * 5, 8 * 33 and 8 * 1025 elements with gaps of
    1000s between them; each segment's maximum sits in its last (first) 8 elements, the middle segment holds the larger values.
    Per segment: amax exact, scale == 448 / amax in f32 exactly, the bytes of quant_ref; the gaps of the destination untouched."""
    from kvq._ffi import check, lib, stream_ptr
    lens, offs, tops = [40, 264, 8200], [16, 80, 368], [3.0, 60.0, 5.0]
    total = 368 + 8200 + 24
    g = torch.Generator().manual_seed(len(where) + periodic)
    src = torch.full((total,), 1000.0, dtype=BF16)
    for s, (n, o, top) in enumerate(zip(lens, offs, tops)):
        seg = ((torch.rand(n, generator=g) * 2 - 1) * (50.0 if s == 1 else 1.0)).to(BF16)
        seg[n - 3 if where == "last 8" else 5] = -top if s == 2 else top
        src[o:o + n] = seg
    dst = torch.full((total,), BYTE_CANARY, dtype=torch.uint8, device="cuda")
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")
    off, n = t64(offs), t64(lens)
    amax, scale = torch.full((3,), -1.0, device="cuda"), torch.full((3,), -1.0, device="cuda")
    sd = src.cuda()
    if periodic:
        step = t64([8, 0, 0, 0])                                    # a multiple of the period: a refresh step
        check(lib().kvq_fp8_quantize_segments_periodic(sd.data_ptr(), off.data_ptr(), n.data_ptr(), 3, max(lens), dst.data_ptr(), amax.data_ptr(),
                                                       scale.data_ptr(), step.data_ptr(), 4, stream_ptr()), "periodic")
    else:
        check(lib().kvq_fp8_quantize_segments(sd.data_ptr(), off.data_ptr(), n.data_ptr(), 3, max(lens), dst.data_ptr(), amax.data_ptr(),
                                              scale.data_ptr(), stream_ptr()), "segments")
    torch.cuda.synchronize()
    got, inside = dst.cpu(), torch.zeros(total, dtype=torch.bool)
    for s, (ln, o, top) in enumerate(zip(lens, offs, tops)):
        assert float(amax[s]) == top == F8.amax_ref(src[o:o + ln]), f"segment {s}: amax {float(amax[s])}, wanted {top}"
        want_scale = torch.tensor(448.0, dtype=torch.float32) / torch.tensor(top, dtype=torch.float32)
        assert torch.equal(scale[s].cpu(), want_scale), f"segment {s}: scale"
        bad, first = F8.quant_report(got[o:o + ln], F8.quant_ref(src[o:o + ln], want_scale, F8.E4M3), F8.E4M3)
        assert bad == 0, f"segment {s}: {bad} bytes differ; first (index, got, want): {first}"
        inside[o:o + ln] = True
    assert bool((got[~inside] == BYTE_CANARY).all()), "bytes written outside the segments"


# ---------------------------------------------------------------------------------------------------------------
# scale update over several records
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,fmt", SELF_ENTRIES, ids=["plain", "e4m3", "e5m2"])
def test_scale_update_over_three_records(ops, entry, fmt):
    """kvq_fp8_update_scales[_fmt] with nsites = 3: the two visited records get max(fmt) / (headroom amax) -- against the f64 value
    to 2^-22 relative (two f32 roundings: the product and the quotient, 2^-24 each, and the slack of one more); the record
    between them saw nothing and keeps its scale bit for bit; all partials are cleared; headroom = 0 only clears."""
    from kvq._ffi import check, lib, stream_ptr
    from kvq import nnops

    def update(st, headroom):
        if entry is None:
            check(lib().kvq_fp8_update_scales(st.data_ptr(), 3, headroom, stream_ptr()), "update")
        else:
            check(lib().kvq_fp8_update_scales_fmt(st.data_ptr(), 3, headroom, nnops.FP8_FORMATS[entry], stream_ptr()), "update_fmt")
        torch.cuda.synchronize()

    def records():
        st = _state(0.0, sites=3)
        st[:, 0] = torch.tensor([11.0, 0.12345678, 7.0])
        st[0, 8 + 5], st[0, 8 + 4095] = 3.7, 11.3                    # the maximum in the record's last slot
        st[2, 8 + 0], st[2, 8 + 2049] = 0.0131, 0.0007               # ... and in its first
        return st

    st = records()
    before = st.cpu().clone()
    update(st, 4.0)
    after = st.cpu()
    for rec, amax in ((0, before[0, 8:].max()), (2, before[2, 8:].max())):
        want = F8.FMT_MAX[fmt] / (4.0 * float(amax.double()))
        assert abs(float(after[rec, 0].double()) - want) <= 2.0 ** -22 * want, (rec, float(after[rec, 0]), want)
    assert torch.equal(after[1, 0].view(torch.int32), before[1, 0].view(torch.int32))
    assert float(after[:, 8:].abs().max()) == 0.0 and float(after[:, 1:8].abs().max()) == 0.0
    st = records()
    update(st, 0.0)
    after = st.cpu()
    assert torch.equal(after[:, 0].view(torch.int32), before[:, 0].view(torch.int32)) and float(after[:, 8:].abs().max()) == 0.0
