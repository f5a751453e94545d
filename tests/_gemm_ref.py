"""Exact f64 references, case generators and judges for the bf16 GEMM family (csrc/kvq_gemm2.hip, csrc/kvq_gemm_any.hip) and its
fused GELU / GELU' / softmax-statistics epilogues (tests/test_gemm_exact_gpu.py).  Everything here runs on the CPU;
tests/test_gemm_ref.py shows that each judge accepts a plain f32 restatement of the kernel's contract and rejects planted mistakes.

The contract (epilogue() of kvq_gemm2.hip, gemm_any_kernel): f32 accumulation, v = acc + bias in f32, ONE rounding to bf16 (RNE);
with accumulate the old bf16 C is added to that rounded value in f32 and the sum is rounded once more.

Why bit-exactness is provable: the operands are integers in [-8, 8] without 0 times a power of two.  With q the product of the two
operands' quanta, every product a*b, the bias and the old C are integer multiples of q, and when
    S = |A| . |B| + |bias| + |C_old| < 2^24 q      (elementwise)
every partial sum of every grouping is an integer multiple of q below 2^24 q in magnitude: exact in f32, whatever order the
hardware adds in.  The stored value must then be bf16_rne(A.B + bias) bit for bit."""
import math
from dataclasses import dataclass
from typing import Optional

import torch

import _pointwise_ref as R

LAYOUTS = ("nt", "nn", "tn")
PAD_LD, PAD_OFF = 24, 8            # a padded parent: row stride = width + 24, the view starts 8 columns (16 bytes) in
BF16 = torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
def in_parent(t, fill=float("nan")):
    """t [r, c] as a view [:, 8:8+c] of a parent [r, c + 24] filled with `fill` (NaN: an operand read outside the view poisons
    whatever it reaches)."""
    r, c = t.shape
    parent = torch.full((r, c + PAD_LD), fill, dtype=t.dtype)
    view = parent[:, PAD_OFF:PAD_OFF + c]
    view.copy_(t)
    return view


def on_device(t, device="cuda"):
    """A device copy of t with the same strides and storage offset (its whole parent travels with it)."""
    if t is None:
        return None
    base = t._base if t._base is not None else t
    return base.to(device).as_strided(t.shape, t.stride(), t.storage_offset())


@dataclass
class Case:
    layout: str
    M: int
    N: int
    K: int
    A: torch.Tensor                    # logical [M, K], f64
    B: torch.Tensor                    # logical [K, N], f64
    a: torch.Tensor                    # bf16, as the layout keeps it in memory (nt / nn: [M, K]; tn: [K, M])
    b: torch.Tensor                    # bf16 (nt: [N, K]; nn / tn: [K, N])
    bias: Optional[torch.Tensor]       # bf16 [N]
    c_old: Optional[torch.Tensor]      # bf16 [M, N]


def make_case(layout, M, N, K, seed, bias=False, accumulate=False, padded=False, ea=0, eb=0, ebias=None):
    """Operands int_values * 2^ea / 2^eb in the memory layout of `layout`; bias int_values * 2^ebias (default ea + eb); old C
    int_values * 2^(ea + eb + 0..5), the exponent drawn per element (bf16-exact; magnitudes up to those of the product's bulk)."""
    assert layout in LAYOUTS
    A = R.int_values((M, K), seed).double() * 2.0 ** ea
    B = R.int_values((K, N), seed + 1).double() * 2.0 ** eb
    a_mem = A.t() if layout == "tn" else A
    b_mem = B.t() if layout == "nt" else B
    put = (lambda t: in_parent(t.to(BF16).contiguous())) if padded else (lambda t: t.to(BF16).contiguous())
    bv = cv = None
    if bias:
        bv = (R.int_values((N,), seed + 2).double() * 2.0 ** (ea + eb if ebias is None else ebias)).to(BF16)
    if accumulate:
        g = torch.Generator().manual_seed(int(seed) + 4)
        ex = torch.randint(0, 6, (M, N), generator=g).double()
        cv = (R.int_values((M, N), seed + 3).double() * 2.0 ** (ea + eb) * 2.0 ** ex).to(BF16)
    c = Case(layout, M, N, K, A, B, put(a_mem), put(b_mem), bv, cv)
    assert torch.equal(logical(c.a, layout, "a"), A) and torch.equal(logical(c.b, layout, "b"), B)      # bf16 holds them exactly
    return c


def logical(t, layout, which):
    """The logical f64 [M, K] (which = "a") or [K, N] ("b") of an operand kept in `layout`'s memory order."""
    t = t.double()
    if which == "a":
        return t.t() if layout == "tn" else t
    return t.t() if layout == "nt" else t


def pick_exponent(y, target):
    """The power of two e for which max|y| * 2^e is nearest (in ratio) to `target`."""
    return int(round(math.log2(target / float(y.abs().max()))))


# ---------------------------------------------------------------------------------------------------------------
# exactness condition and the reference
# ---------------------------------------------------------------------------------------------------------------
def quantum(t):
    """The largest power of two that divides every non-zero value of t (f64)."""
    x = t.double().abs().reshape(-1)
    x = x[x > 0]
    assert x.numel() and bool(torch.isfinite(x).all())
    q = 2.0 ** math.floor(math.log2(float(x.min())))
    for _ in range(64):
        if bool(torch.all(x / q == torch.round(x / q))):
            return q
        q *= 0.5
    raise AssertionError("no power-of-two quantum")


def assert_gemm_exact_range(A, B, bias=None, C_old=None):
    """S = |A| . |B| (+ |bias|) (+ |C_old|) < 2^24 q elementwise, q = quantum(A) * quantum(B), bias and C_old multiples of q:
    every partial sum of A.B + bias in ANY grouping, and the f32 addition of the old C to the rounded product, are exact in f32.
    On the operands, not on the result: a sum whose grouping we do not control can leave the range on the way to a small result.
    A [M, K], B [K, N] logical (any float dtype).  Returns (max S / q, q)."""
    A, B = A.double(), B.double()
    q = quantum(A) * quantum(B)
    # K max|A| max|B| bounds every element of |A| . |B|: when that bound passes, so does S (large cases skip the second matmul)
    S = torch.tensor(A.shape[1] * float(A.abs().max()) * float(B.abs().max()), dtype=torch.float64)
    if float(S) + sum(float(e.double().abs().max()) for e in (bias, C_old) if e is not None) >= R.EXACT_LIMIT * q:
        S = A.abs() @ B.abs()
    for extra in (bias, C_old):
        if extra is not None:
            e = extra.double()
            assert bool(torch.all(e / q == torch.round(e / q))), "GEMM case leaves the exact f32 range: bias / old C is no multiple of the products' quantum"
            S = S + e.abs()
    top = float(S.max()) / q
    assert top < R.EXACT_LIMIT, f"GEMM case leaves the exact f32 range: max S / q = {top:.0f} >= 2^24"
    assert q >= 2.0 ** -100 and float(S.max()) < 2.0 ** 100, "GEMM case leaves the normal f32 range"
    return top, q


def case_exact_range(c):
    return assert_gemm_exact_range(c.A, c.B, c.bias, c.c_old)


def rne_bf16(x64):
    """bf16 RNE of f64 values that are exact in f32 (one rounding)."""
    f = x64.float()
    assert torch.equal(f.double(), x64), "reference value is not exact in f32"
    return f.to(BF16)


def gemm_ref(A, B, bias=None, C_old=None):
    """(y, final, want): y = A.B (+ bias) in f64 (exact: integers below 2^53 times a power of two); final = the f64 value whose
    single RNE rounding the kernel must store -- y itself, or bf16_rne(y) + C_old with accumulate (the two-rounding chain);
    want = that rounding, bf16."""
    y = A.double() @ B.double()
    if bias is not None:
        y = y + bias.double()[None, :]
    final = y if C_old is None else rne_bf16(y).double() + C_old.double()
    return y, final, rne_bf16(final)


def case_ref(c):
    return gemm_ref(c.A, c.B, c.bias, c.c_old)


# ---------------------------------------------------------------------------------------------------------------
# judges
# ---------------------------------------------------------------------------------------------------------------
def exact_report(out, final, limit=5):
    """(count, first few (row, col, got, want)) of the elements of bf16 `out` that are not the RNE rounding of `final`."""
    bad = R.judge_exact(out, final)
    if not bad:
        return 0, []
    o = out.detach().cpu()
    want = final.float().to(BF16)
    diff = (R.bf16_bits(o) != R.bf16_bits(want)) & ~((o.float() == 0) & (want.float() == 0))
    idx = diff.nonzero()[:limit].tolist()
    return bad, [(r, k, float(o[r, k]), float(want[r, k])) for r, k in idx]


def assert_exact(out, final, what):
    bad, first = exact_report(out, final)
    assert bad == 0, f"{what}: {bad} of {out.numel()} elements are not bf16_rne of the exact value; first (row, col, got, want): {first}"


def gelu_epilogue_ratio(a_out, h_stored):
    """Per element |a_out - gelu(h)| over the forward bf16 envelope, h = the bf16 value the kernel stored (<= 1 passes)."""
    h = h_stored.detach().cpu()
    return R.gelu_bf16_ratio(a_out, h.double(), R.gelu_ref(h)[0], False)


def dgelu_epilogue_ratio(out, g, h):
    """Per element |out - g gelu'(h)| over 2^-8 |g gelu'(h)| + |g| delta (1 + |h|) + 2^-126: the backward envelope of
    _pointwise_ref scaled by |g|, g = bf16_rne(A.B) known exactly (<= 1 passes)."""
    d = R.gelu_delta()[0]
    g, h = g.detach().cpu().double(), h.detach().cpu().double()
    ref = g * R.gelu_ref(h)[1]
    env = ref.abs() * 2.0 ** -8 + g.abs() * d * (1.0 + h.abs()) + R.TINY
    return (out.detach().cpu().double() - ref).abs() / env


def all_h_values(M, N, seed, bound=8.0):
    """bf16 [M, N] that holds every finite bf16 value of |h| <= bound at least once (shuffled; the rest are repeats)."""
    xs, fin = R.all_bf16_values()
    vals = xs[fin & (xs.float().abs() <= bound)]
    assert vals.numel() <= M * N
    g = torch.Generator().manual_seed(int(seed))
    fill = vals[torch.randint(0, vals.numel(), (M * N - vals.numel(),), generator=g)]
    flat = torch.cat([vals, fill])[torch.randperm(M * N, generator=g)]
    return flat.reshape(M, N).contiguous()


def dgelu_part_check(part, out_stored, bm):
    """part [ceil(M / bm), N] f32 against the f64 column sums of the STORED bf16 out over each row tile: the worst
    |part - sum| / ((bm - 1) 2^-24 sum|out|) (at most bm - 1 f32 additions of partial sums bounded by sum|out|, half an ulp each)."""
    o = out_stored.detach().cpu().double()
    p = part.detach().cpu().double()
    M = o.shape[0]
    assert p.shape == (-(-M // bm), o.shape[1])
    worst = 0.0
    for t in range(p.shape[0]):
        blk = o[t * bm:(t + 1) * bm]
        bound = (bm - 1) * 2.0 ** -24 * blk.abs().sum(0)
        err = (p[t] - blk.sum(0)).abs()
        bad = err > bound
        if bool(bad.any()):
            return float("inf")
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    return worst


def ce_stats_judge(stats, logits_stored, V, tile=256):
    """The LM-head epilogue's per-(row, 256-column tile) statistics against the stored logits.  Returns a dict:
    max_bad / arg_bad: tiles whose maximum (by value) / first arg-max (int bits) differ from ce_tile_stats;
    pad_bad: wholly padded tiles that are not (-inf, 0, INT_MAX);
    ratio [rows, live tiles]: |m + log(sum) - lse_tile| / (2^-20 max(1, |lse_tile|, max|x|)), lse_tile in f64 (ce_row_ratio)."""
    st = stats.detach().cpu()
    x = logits_stored.detach().cpu().double()
    n, tiles = st.shape[0], st.shape[1]
    want = R.ce_tile_stats(x, V, tiles, tile)
    bits = lambda t: t.contiguous().view(torch.int32)
    live = [t for t in range(tiles) if t * tile < V]
    dead = [t for t in range(tiles) if t * tile >= V]
    res = dict(max_bad=int((st[:, live, 0] != want[:, live, 0]).sum()),
               arg_bad=int((bits(st[:, :, 2])[:, live] != bits(want[:, :, 2])[:, live]).sum()), pad_bad=0)
    for t in dead:
        ok = (st[:, t, 0] == -math.inf) & (st[:, t, 1] == 0) & (bits(st[:, t, 2]) == R.INT_MAX)
        res["pad_bad"] += int((~ok).sum())
    ratios = []
    for t in live:
        seg = x[:, t * tile:min((t + 1) * tile, V)]
        ref = dict(lse=torch.logsumexp(seg, dim=1), absmax=seg.abs().max(dim=1).values)
        got = st[:, t, 0].double() + torch.log(st[:, t, 1].double())
        ratios.append(R.ce_row_ratio(got, ref["lse"], ref))
    res["ratio"] = torch.stack(ratios, dim=1)
    return res
