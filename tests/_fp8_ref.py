"""Exact f64 references, case generators and judges for the fp8 GEMMs (gemm2_f8_kernel of csrc/kvq_gemm2.hip: kvq_gemm_fp8_nt,
kvq_gemm_fp8_nt_ex, kvq_gemm_fp8_nt_gelu) and the quantisation passes (csrc/kvq_fp8.hip; quant8 / quant8_fmt / amax8 of
csrc/kvq_common.h), used by tests/test_fp8_exact_gpu.py.  Everything here runs on the CPU; tests/test_fp8_ref.py shows that the
tables equal torch's float8 types, that quant_ref equals torch's conversion on every bf16 pattern, and that each judge accepts a plain
f32 restatement of the kernels' contract and rejects planted mistakes.  The bf16 machinery is tests/_gemm_ref.py's, not copied.

The GEMM contract: acc = A8 . B8^T in f32 on the matrix cores, mul = 1 / (sa sb) in f32, v = acc * mul + bias in f32, ONE rounding to
bf16 (RNE); with accumulate the old bf16 C is added to that rounded value in f32 and the sum is rounded once more.

Why bit-exactness is provable (power-of-two scales): the operands are integers in [-8, 8] without 0 times a power of two -- exact in
e4m3 and in e5m2 (three significant bits).  With q the product of the operands' quanta every product is a multiple of q, and while
S = |A| . |B| < 2^24 q every partial sum of every grouping is exact in f32 (assert_gemm_exact_range); the cases stay below 2^17 q, so
that an accumulator narrower than f32 by up to seven bits would still be exact.  mul is a power of two: acc * mul is exact, and
acc * mul + bias is one exact value whether the compiler contracts it or not (bias and old C are multiples of q mul).

Scales that are no powers of two: mul carries three f32 roundings (sa sb, the reciprocal, acc * mul) and the sum one; the stored
value must lie between the roundings of v -+ (2^-22 |acc / (sa sb)| + 2^-24 |v|)."""
import functools
import math
from dataclasses import dataclass
from typing import Optional

import torch

import _gemm_ref as G
import _pointwise_ref as R

BF16 = torch.bfloat16
E4M3, E5M2 = "e4m3", "e5m2"
FORMATS = (E4M3, E5M2)
FMT_MAX = {E4M3: 448.0, E5M2: 57344.0}
FMT_TORCH = {E4M3: torch.float8_e4m3fn, E5M2: torch.float8_e5m2}
N_FINITE = {E4M3: 0x7F, E5M2: 0x7C}            # codes 0 .. N_FINITE - 1 are the finite non-negative values, in increasing order
NAN_BYTE = 0x7F                                # a NaN in both formats: what a padded parent is filled with
PAD8_LD, PAD8_OFF = 32, 16                     # a padded parent of bytes: row stride = K + 32, the view starts 16 bytes in
ACC_LIMIT = 1 << 17                            # S / q of every exact case stays below this


# ---------------------------------------------------------------------------------------------------------------
# the two formats
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def decode_table(fmt):
    """f64 [256]: the value of every byte of OCP e4m3fn (4 exponent bits, bias 7, no inf, NaN = 0x7F / 0xFF) or e5m2 (5 exponent
    bits, bias 15, inf = 0x7C / 0xFC, NaN = 0x7D .. 0x7F / 0xFD .. 0xFF), from the bit fields."""
    assert fmt in FORMATS
    ebits, mbits, bias = (4, 3, 7) if fmt == E4M3 else (5, 2, 15)
    vals = []
    for byte in range(256):
        sign = -1.0 if byte & 0x80 else 1.0
        e = (byte >> mbits) & ((1 << ebits) - 1)
        m = byte & ((1 << mbits) - 1)
        if fmt == E4M3 and e == 15 and m == 7:
            v = math.nan
        elif fmt == E5M2 and e == 31:
            v = sign * math.inf if m == 0 else math.nan
        elif e == 0:
            v = sign * m * 2.0 ** (1 - bias - mbits)               # subnormal (and +-0)
        else:
            v = sign * (1.0 + m / (1 << mbits)) * 2.0 ** (e - bias)
        vals.append(v)
    return torch.tensor(vals, dtype=torch.float64)


def decode(byte, fmt):
    """f64 values of uint8 bytes (any shape)."""
    return decode_table(fmt)[byte.detach().cpu().long()]


def encode_exact(v, fmt):
    """The bytes of f64 values that are exactly representable in fmt (asserted)."""
    pos = decode_table(fmt)[:N_FINITE[fmt]]
    mag = v.double().abs()
    code = torch.searchsorted(pos, mag).clamp_max(N_FINITE[fmt] - 1)
    assert torch.equal(pos[code], mag), f"a value is not exact in {fmt}"
    return (code | torch.where(torch.signbit(v.double()), 0x80, 0)).to(torch.uint8)


def quant_ref(x_bf16, scale_f32, fmt):
    """The bytes the quantisation kernels must write for bf16 x under an f32 scale: p = f32(x) * scale (one f32 rounding); a NaN
    stays a NaN (byte 0x7F here: judge it with quant_report, by "decodes to NaN"); anything else is clamped to +-max(fmt), so
    +-inf saturates; round to nearest even with subnormals, by search in the decode table in f64; -0 and negative values that
    round to zero keep their sign."""
    x = x_bf16.detach().cpu()
    assert x.dtype == BF16
    s = torch.as_tensor(scale_f32, dtype=torch.float32).detach().cpu().reshape(())
    p = x.float() * s
    nan = torch.isnan(p)
    mag = p.double().abs().clamp_max(FMT_MAX[fmt])
    mag = torch.where(nan, torch.zeros_like(mag), mag)
    pos = decode_table(fmt)[:N_FINITE[fmt]]
    hi = torch.searchsorted(pos, mag).clamp_max(N_FINITE[fmt] - 1)          # the first code whose value is >= |p|
    lo = (hi - 1).clamp_min(0)
    dlo, dhi = mag - pos[lo], pos[hi] - mag
    code = torch.where((dhi < dlo) | ((dhi == dlo) & (hi % 2 == 0)), hi, lo)  # nearest; a tie goes to the even code
    code = torch.where(nan, torch.full_like(code, NAN_BYTE), code)
    return (code | torch.where(torch.signbit(p), 0x80, 0)).to(torch.uint8)


def quant_report(got, want, fmt, limit=5):
    """(count, first few (flat index, got byte, wanted byte)) of the bytes that differ from quant_ref's; where a NaN is wanted any
    byte that decodes to NaN passes."""
    got, want = got.detach().cpu().reshape(-1), want.detach().cpu().reshape(-1)
    assert got.dtype == torch.uint8 and got.shape == want.shape
    want_nan = torch.isnan(decode(want, fmt))
    ok = torch.where(want_nan, torch.isnan(decode(got, fmt)), got == want)
    idx = (~ok).nonzero().reshape(-1)
    return int(idx.numel()), [(int(i), int(got[i]), int(want[i])) for i in idx[:limit]]


def amax_ref(x_bf16):
    """max |x| over the elements that are no NaN (f32 value; inf when an inf is there; 0 for an empty maximum)."""
    a = x_bf16.detach().cpu().float().abs()
    a = a[~torch.isnan(a)]
    return float(a.max()) if a.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------
# GEMM cases
# ---------------------------------------------------------------------------------------------------------------
def in_parent8(t):
    """uint8 t [r, K] as the view [:, 16:16+K] of a parent [r, K + 32] filled with 0x7F (NaN in both formats: an operand byte
    read outside the view poisons whatever it reaches)."""
    r, c = t.shape
    parent = torch.full((r, c + PAD8_LD), NAN_BYTE, dtype=torch.uint8)
    view = parent[:, PAD8_OFF:PAD8_OFF + c]
    view.copy_(t)
    return view


def is_pow2(x):
    return x > 0 and math.frexp(x)[0] == 0.5


@dataclass
class Case8:
    M: int
    N: int
    K: int
    a_fmt: str
    A: torch.Tensor                    # logical [M, K], f64: the decoded a8
    B: torch.Tensor                    # logical [K, N], f64: the decoded b8 (e4m3)
    a8: torch.Tensor                   # uint8 [M, K]
    b8: torch.Tensor                   # uint8 [N, K]
    sa: torch.Tensor                   # f32 scalars: the device scales
    sb: torch.Tensor
    mul: float                         # 1 / (sa sb) in f64 from the f32 scales (exact when both are powers of two)
    q: float                           # the product quantum 2^(ea + eb)
    bias: Optional[torch.Tensor]       # bf16 [N]
    c_old: Optional[torch.Tensor]      # bf16 [M, N]

    @property
    def exact(self):
        return is_pow2(float(self.sa)) and is_pow2(float(self.sb))


def make_case8(M, N, K, seed, a_fmt=E4M3, bias=False, accumulate=False, padded=False, ea=0, eb=0, sa=8.0, sb=0.25, unit=False):
    """Operands int_values * 2^ea (a_fmt) and * 2^eb (e4m3), kept as bytes in NT memory order; unit: operands in {-1, 1} * 2^e
    instead (S <= K).  sa, sb: the device scales.  bias = int_values * q mul, old C = int_values * q mul * 2^(0..5) drawn per
    element, q = 2^(ea + eb), mul = 1 / (sa sb): bf16-exact multiples of the scaled product quantum when the scales are powers of
    two, rounded to bf16 otherwise (then only the interval judge applies, and there is no old C)."""
    assert a_fmt in FORMATS and K % 128 == 0
    ia, ib = R.int_values((M, K), seed), R.int_values((K, N), seed + 1)
    if unit:
        ia, ib = torch.sign(ia), torch.sign(ib)
    A, B = ia.double() * 2.0 ** ea, ib.double() * 2.0 ** eb
    a8, b8 = encode_exact(A, a_fmt), encode_exact(B.t().contiguous(), E4M3)
    assert torch.equal(decode(a8, a_fmt), A) and torch.equal(decode(b8, E4M3).t(), B)
    if padded:
        a8, b8 = in_parent8(a8), in_parent8(b8)
    sa32, sb32 = torch.tensor(sa, dtype=torch.float32), torch.tensor(sb, dtype=torch.float32)
    mul = 1.0 / (float(sa32) * float(sb32))
    q = 2.0 ** (ea + eb)
    pow2 = is_pow2(float(sa32)) and is_pow2(float(sb32))
    bv = cv = None
    if bias:
        b64 = R.int_values((N,), seed + 2).double() * q * mul
        bv = b64.float().to(BF16)
        assert not pow2 or torch.equal(bv.double(), b64)
    if accumulate:
        assert pow2, "an old C needs the exact judge"
        g = torch.Generator().manual_seed(int(seed) + 4)
        ex = torch.randint(0, 6, (M, N), generator=g).double()
        c64 = R.int_values((M, N), seed + 3).double() * q * mul * 2.0 ** ex
        cv = c64.float().to(BF16)
        assert torch.equal(cv.double(), c64)
    return Case8(M, N, K, a_fmt, A, B, a8, b8, sa32, sb32, mul, q, bv, cv)


def case8_exact_range(c):
    """The exactness condition, on the decoded operands, before every launch.  Power-of-two scales: S = |A| . |B| + |bias| / mul +
    |C_old| / mul < 2^17 q with bias / mul and C_old / mul multiples of q (assert_gemm_exact_range of tests/_gemm_ref.py, in units
    of the unscaled accumulator).  Otherwise: |A| . |B| < 2^17 q alone -- the accumulator is exact, the epilogue is judged by an
    interval.  Returns (max S / q, q)."""
    if c.exact:
        top, q = G.assert_gemm_exact_range(c.A, c.B, None if c.bias is None else c.bias.double() / c.mul,
                                           None if c.c_old is None else c.c_old.double() / c.mul)
    else:
        assert c.c_old is None
        top, q = G.assert_gemm_exact_range(c.A, c.B)
    assert q == c.q and top < ACC_LIMIT, f"fp8 GEMM case: max S / q = {top:.0f} >= 2^17"
    return top, q


def case8_ref(c):
    """(y, final, want) as gemm_ref of tests/_gemm_ref.py for y = (A . B) mul + bias; power-of-two scales only."""
    assert c.exact
    return G.gemm_ref(c.A * c.mul, c.B, c.bias, c.c_old)


# ---------------------------------------------------------------------------------------------------------------
# interval judge: scales that are no powers of two
# ---------------------------------------------------------------------------------------------------------------
def rne_bf16_f64(x):
    """bf16 RNE of f64 values in ONE rounding (through f32 there would be two).  Normal bf16 range only (asserted)."""
    x = x.double()
    m, e = torch.frexp(x.abs())                                       # |x| = m 2^e, m in [0.5, 1): the bf16 spacing is 2^(e - 8)
    assert int(e.min()) > -100 and int(e.max()) < 100
    r = torch.ldexp(torch.round(torch.ldexp(x, 8 - e)), e - 8)        # torch.round: half to even
    out = r.float().to(BF16)
    assert torch.equal(out.double(), r)
    return out


def interval_ref(c, max_two_valued=0.01):
    """(lo, hi, share): the stored bf16 must lie in [lo, hi] = [bf16_rne(v - d), bf16_rne(v + d)], v = acc / (sa sb) + bias in f64
    from the f32 scales, d = 2^-22 |acc / (sa sb)| + 2^-24 |v| (three f32 roundings on the way to mul * acc, one for the sum).
    share = the part of the elements with lo != hi; asserted to be at most 1 %, a condition on the case, not a measurement."""
    assert c.c_old is None
    acc = c.A @ c.B
    s = acc / (c.sa.double() * c.sb.double())
    v = s + (c.bias.double()[None, :] if c.bias is not None else 0.0)
    d = 2.0 ** -22 * s.abs() + 2.0 ** -24 * v.abs()
    lo, hi = rne_bf16_f64(v - d), rne_bf16_f64(v + d)
    share = float((lo.float() != hi.float()).double().mean())
    assert share <= max_two_valued, f"{share:.4%} of the elements have two admissible values"
    return lo, hi, share


def interval_report(out, lo, hi, limit=5):
    """(count, first few (row, col, got, lo, hi)) of the elements of bf16 `out` outside [lo, hi] (a NaN is outside)."""
    o = out.detach().cpu().float()
    bad = ~((o >= lo.float()) & (o <= hi.float()))
    idx = bad.nonzero()[:limit].tolist()
    return int(bad.sum()), [(r, k, float(o[r, k]), float(lo[r, k]), float(hi[r, k])) for r, k in idx]


def assert_interval(out, lo, hi, what):
    bad, first = interval_report(out, lo, hi)
    assert bad == 0, f"{what}: {bad} of {out.numel()} elements outside their interval; first (row, col, got, lo, hi): {first}"


# ---------------------------------------------------------------------------------------------------------------
# single-product cases: every byte pattern of an operand
# ---------------------------------------------------------------------------------------------------------------
ONE_HOT_K, ONE_HOT_OTHER = 256, 72


def one_hot_case(fmt, slot):
    """slot "a": A8 [256, 256] in fmt holds byte pattern i at (i, i mod K) and zero bytes elsewhere, B8 [72, 256] (e4m3) holds the
    powers of two 2^((j + 2 k) mod 5 - 2) at (j, k): out[i, j] = decode(i) * B[j, i], one non-zero product per output (none for
    the two zero patterns).  slot "b" (fmt e4m3): the same with the operands exchanged, out[j, i].  Scales 4 and 1/2.
    Returns (case, want): want f64 [M, N] -- exact in bf16 whatever the adder does; NaN where the pattern is a NaN, +-inf where it
    is an e5m2 inf."""
    assert slot in ("a", "b") and (slot == "a" or fmt == E4M3)
    K, J = ONE_HOT_K, ONE_HOT_OTHER
    i = torch.arange(256)
    swept = torch.zeros((256, K), dtype=torch.uint8)
    swept[i, i % K] = i.to(torch.uint8)
    jj, kk = torch.meshgrid(torch.arange(J), torch.arange(K), indexing="ij")
    other = 2.0 ** (((jj + 2 * kk) % 5) - 2).double()
    other8 = encode_exact(other, E4M3)
    prod = decode_table(fmt)[:, None] * other[:, i % K].t()            # [256, J]: decode(i) * other[j, i mod K]
    sa, sb = torch.tensor(4.0), torch.tensor(0.5)
    mul = 0.5
    if slot == "a":
        c = Case8(256, J, K, fmt, decode(swept, fmt), other.t(), swept, other8, sa, sb, mul, 0.0, None, None)
        return c, prod * mul
    c = Case8(J, 256, K, E4M3, other, decode(swept, fmt).t(), other8, swept, sa, sb, mul, 0.0, None, None)
    return c, prod.t() * mul


def one_hot_report(out, want, limit=5):
    """(count, first few (row, col, got, want)): NaN where want is NaN; elsewhere the bits of want (exact in bf16; +-0 are equal)."""
    o = out.detach().cpu()
    w = want.float().to(BF16)
    nan = torch.isnan(want)
    assert torch.equal(torch.where(nan, torch.zeros_like(want), w.double()), torch.where(nan, torch.zeros_like(want), want))
    same = (R.bf16_bits(o) == R.bf16_bits(w)) | ((o.float() == 0) & (w.float() == 0))
    ok = torch.where(nan, torch.isnan(o.float()), same)
    idx = (~ok).nonzero()[:limit].tolist()
    return int((~ok).sum()), [(r, k, float(o[r, k]), float(want[r, k])) for r, k in idx]
