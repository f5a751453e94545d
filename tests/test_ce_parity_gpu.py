"""Per-row and per-element parity of the reconstruction-loss kernels (csrc/kvq_ce.hip) against f64 from the up-cast logits:
row_lse, row_loss, pred (first arg-max) and the gradient c (softmax - onehot), at every byte misalignment of a row and with the
target / the maximum placed on each part of the head | 16-byte vectors | tail walk; exact ties; large shifts, wide spreads and
-inf logits; and kvq_ce_forward_stats on statistics built directly.

Bounds: |lse - ref| and |row_loss - ref| <= 2^-20 M with M = max(1, |lse_ref|, max |x|) (eight f32 ulps at magnitude M: the kernel
forms m + logf(s) and then lse - x_t, an ulp of M each, and __expf scales its argument by log2 e in f32); gradient rtol 2e-5, atol
1e-8 per element, plus one bf16 ulp 2^-8 |ref| for bf16 storage, plus -- on the target's column and in rows of magnitude M > 21
only -- the c p 2^-20 M that the allowed error of the stored f32 lse puts on p (tests/_pointwise_ref.py: ce_grad_ratio).  Measured worst ratios: profiles/pointwise_parity.md."""
import math

import pytest
import torch

import _pointwise_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
PAD = 64                      # frame elements around the logits (a multiple of 16 bytes in both dtypes)
FRAME = 3.0
N_ROWS = 9
G_LOSS = 1.7


@pytest.fixture(scope="module")
def lib():
    from kvq import _ffi
    _ffi.lib()
    assert torch.cuda.is_available()
    return _ffi.lib()


class Case:
    """Logits x [N, V] (CPU, in `dtype`) placed in a flat framed buffer at storage offset o with row stride ld."""

    def __init__(self, x, target, dtype, o, ld):
        self.N, self.V = x.shape
        self.dtype, self.o, self.ld = dtype, o, ld
        self.io = 0 if dtype == F32 else 1
        self.x = x.to(dtype)
        self.target = target.long()
        self.span = self.N * ld
        flat = torch.full((PAD + o + self.span + PAD,), FRAME, dtype=dtype)
        flat[PAD + o:PAD + o + self.span].view(self.N, ld)[:, :self.V] = self.x
        self.flat = flat.cuda()
        assert self.flat.data_ptr() % 16 == 0

    def ptr(self, flat):
        return flat.data_ptr() + (PAD + self.o) * flat.element_size()

    def rows(self, flat):
        return flat[PAD + self.o:PAD + self.o + self.span].view(self.N, self.ld)

    def outside_untouched(self, flat, snap):
        a, b = PAD + self.o, PAD + self.o + self.span
        return torch.equal(flat[:a], snap[:a]) and torch.equal(flat[b:], snap[b:])


def walks(dtype, o, ld, V, N=N_ROWS):
    """(head, nvec, tail0) per row for a view at storage offset o of a 16-byte aligned buffer (PAD keeps the alignment)."""
    sz = 4 if dtype == F32 else 2
    return [R.row_walk(4096 + o * sz, n, V, ld, sz) for n in range(N)]


def run_and_judge(lib, case, what, figures=None, backward=True):
    """Forward, backward out of place and in place; asserts every per-row and per-element property and returns the f64 reference."""
    from kvq._ffi import check, stream_ptr
    N, V, ld, io = case.N, case.V, case.ld, case.io
    dev = "cuda"
    tgt = case.target.to(dev)
    rl = torch.empty(N, device=dev); lse = torch.empty(N, device=dev); pred = torch.empty(N, dtype=torch.int64, device=dev)
    out = torch.empty(2, device=dev)
    snap = case.flat.clone()
    check(lib.kvq_ce_forward(case.ptr(case.flat), tgt.data_ptr(), N, V, ld, io, rl.data_ptr(), lse.data_ptr(), pred.data_ptr(),
                             out[0:].data_ptr(), out[1:].data_ptr(), stream_ptr()), "kvq_ce_forward")
    assert torch.equal(case.flat, snap), f"{what}: the forward wrote to the logits"
    c = G_LOSS / N
    ref = R.ce_ref(case.x.float(), case.target, c)
    assert torch.all(torch.isfinite(ref["lse"])), "the f64 reference itself must be finite"
    assert torch.equal(pred.cpu(), ref["pred"]), f"{what}: pred {pred.cpu().tolist()} != first arg-max {ref['pred'].tolist()}"
    assert torch.all(torch.isfinite(lse)), f"{what}: lse is not finite: {lse.cpu().tolist()}"
    r_lse = R.ce_row_ratio(lse, ref["lse"], ref)
    r_loss = R.ce_row_ratio(rl, ref["row_loss"], ref)
    fin = torch.isfinite(ref["row_loss"])
    assert torch.all(fin), "targets of the test rows are finite"
    worst = dict(lse=float(r_lse.max()), row_loss=float(r_loss.max()))
    assert worst["lse"] <= 1 and worst["row_loss"] <= 1, f"{what}: lse / row_loss error over 2^-20 M: {worst}"
    # mean loss and accuracy as tests/test_ce_gpu.py judges them; rows of large magnitude (the +-1e4 shifts) bring their own
    # allowed row_loss error 2^-20 M into the mean
    mean_ref = float(ref["row_loss"].mean())
    mean_tol = 1e-6 + 2e-6 * abs(mean_ref) + float(R.ce_large_row_slack(ref).mean())
    assert abs(out[0].item() - mean_ref) <= mean_tol, f"{what}: mean loss {out[0].item()} vs {mean_ref}"
    acc_ref = float((ref["pred"] == case.target).double().mean())
    assert abs(out[1].item() - acc_ref) <= 1e-6 * max(acc_ref, 1e-30) + 1e-9, f"{what}: accuracy"
    if backward:
        gs = torch.full((1,), G_LOSS, device=dev)
        g_flat = torch.full_like(case.flat, FRAME)
        g_snap = g_flat.clone()
        check(lib.kvq_ce_backward(case.ptr(case.flat), tgt.data_ptr(), lse.data_ptr(), gs.data_ptr(), N, V, ld, io, case.ptr(g_flat),
                                  stream_ptr()), "kvq_ce_backward")
        in_flat = case.flat.clone()
        check(lib.kvq_ce_backward(case.ptr(in_flat), tgt.data_ptr(), lse.data_ptr(), gs.data_ptr(), N, V, ld, io, case.ptr(in_flat),
                                  stream_ptr()), "kvq_ce_backward in place")
        assert torch.equal(case.flat, snap), f"{what}: the out-of-place backward wrote to the logits"
        assert case.outside_untouched(g_flat, g_snap) and case.outside_untouched(in_flat, snap), f"{what}: wrote outside the view"
        g = case.rows(g_flat)
        assert torch.equal(g, case.rows(in_flat)), f"{what}: in-place and out-of-place gradients differ"
        assert torch.all(g[:, V:] == 0), f"{what}: padding columns are not zero"
        gv = g[:, :V].cpu()
        assert torch.equal(gv.float().argmin(dim=1), case.target) or V == 1, f"{what}: the -1 is not on the target's column"
        r_g = R.ce_grad_ratio(gv, ref, case.dtype == BF16, case.target)
        worst["grad"] = float(r_g.max())
        assert worst["grad"] <= 1, f"{what}: gradient error / tolerance {worst['grad']:.3f} at {divmod(int(r_g.argmax()), V)}"
    if figures is not None:
        for k, v in worst.items():
            figures[k] = max(figures.get(k, 0.0), v)
    return ref


def _print_figures(name, figures):
    print(f"FIGURE ce {name}: worst ratios " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(figures.items())))


def _base_logits(N, V, seed):
    g = torch.Generator().manual_seed(seed)
    return 2 * torch.randn(N, V, generator=g)


# ---------------------------------------------------------------------------------------------------------------
# a. alignment x target position x maximum position
# ---------------------------------------------------------------------------------------------------------------
VS = [1, 2, 3, 5, 8, 13, 1027, 2 * 256 * 8 + 3]


@pytest.mark.parametrize("dtype,o,pad", [(F32, 0, 0), (F32, 1, 0), (F32, 2, 3), (F32, 3, 3), (F32, 0, 3), (F32, 1, 3), (F32, 2, 0), (F32, 3, 0),
                                         (BF16, 0, 0), (BF16, 1, 0), (BF16, 3, 5), (BF16, 7, 5), (BF16, 0, 5), (BF16, 1, 5), (BF16, 3, 0),
                                         (BF16, 7, 0)])
def test_ce_alignment_target_and_maximum_positions(lib, dtype, o, pad):
    vec = 4 if dtype == F32 else 8
    figures = {}
    for V in VS:
        ld = V + pad
        w = walks(dtype, o, ld, V)
        pos = [R.walk_positions(h, nv, t0, V, vec) for h, nv, t0 in w]
        base = _base_logits(N_ROWS, V, V)
        g = torch.Generator().manual_seed(V + 1)
        rand_t = torch.randint(0, V, (N_ROWS,), generator=g)
        for k in range(max(len(p) for p in pos)):
            at = torch.tensor([p[k % len(p)] for p in pos])
            # the target on that position
            run_and_judge(lib, Case(base, at, dtype, o, ld), f"V={V} ld={ld} o={o} target at {at.tolist()}", figures)
            # the unique maximum on that position
            x = base.clone()
            x[torch.arange(N_ROWS), at] = float(base.max()) + 2.0
            ref = run_and_judge(lib, Case(x, rand_t, dtype, o, ld), f"V={V} ld={ld} o={o} maximum at {at.tolist()}", figures)
            assert torch.equal(ref["pred"], at)
    _print_figures(f"positions {dtype} o={o} ld=V+{pad}", figures)


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("V", [5, 13, 1027, 2 * 256 * 8 + 3])
def test_ce_backward_bias_in_place(lib, dtype, V):
    """kvq_ce_backward_bias in place at ld % 8 == 0, the target on the last real column before the padding."""
    from kvq._ffi import check, stream_ptr
    ld = (V + 7) // 8 * 8
    assert ld > V
    N = 37                                                                # two row blocks of 32, the second one short
    tgt = torch.randint(0, V, (N,), generator=torch.Generator().manual_seed(V))
    tgt[::2] = V - 1
    case = Case(_base_logits(N, V, V + 7), tgt, dtype, 0, ld)
    ref = run_and_judge(lib, case, f"bias V={V}", backward=False)
    dev = "cuda"
    t = tgt.to(dev)
    rl = torch.empty(N, device=dev); lse = torch.empty(N, device=dev); pred = torch.empty(N, dtype=torch.int64, device=dev)
    check(lib.kvq_ce_forward(case.ptr(case.flat), t.data_ptr(), N, V, ld, case.io, rl.data_ptr(), lse.data_ptr(), pred.data_ptr(), None, None,
                             stream_ptr()), "fwd")
    gs = torch.full((1,), G_LOSS, device=dev)
    P = lib.kvq_ce_bwd_partial_rows(N)
    assert P == 2
    part = torch.full((PAD + P * ld + PAD,), FRAME, device=dev)
    snap = case.flat.clone()
    g_flat = case.flat.clone()
    check(lib.kvq_ce_backward_bias(case.ptr(g_flat), t.data_ptr(), lse.data_ptr(), gs.data_ptr(), N, V, ld, case.io, case.ptr(g_flat),
                                   part[PAD:].data_ptr(), P * ld * 4, stream_ptr()), "bwd_bias")
    assert case.outside_untouched(g_flat, snap) and torch.all(part[:PAD] == FRAME) and torch.all(part[PAD + P * ld:] == FRAME)
    g = case.rows(g_flat)
    pr = part[PAD:PAD + P * ld].view(P, ld)
    assert torch.all(g[:, V:] == 0) and torch.all(pr[:, V:] == 0), "padding columns are not zero"
    gv = g[:, :V].cpu()
    assert torch.equal(gv.float().argmin(dim=1), tgt)
    r_g = R.ce_grad_ratio(gv, ref, dtype == BF16, tgt)
    assert float(r_g.max()) <= 1, f"gradient error / tolerance {float(r_g.max()):.3f}"
    st = gv.double()
    for p in range(P):
        blk = st[p * 32:(p + 1) * 32]
        bound = 31 * 2.0 ** -24 * blk.abs().sum(0)                        # at most 31 f32 additions of the stored values
        assert torch.all((pr[p, :V].cpu().double() - blk.sum(0)).abs() <= bound), f"partial row {p} is not the f32 sum of the stored values"


# ---------------------------------------------------------------------------------------------------------------
# b. ties
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("three", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_ce_ties_take_the_first_maximum(lib, dtype, three):
    V, o = 2 * 256 * 8 + 3, 1
    ld = V
    vec = 4 if dtype == F32 else 8
    w = walks(dtype, o, ld, V)
    assert min(nv for _, nv, _ in w) >= 256 + 64 + 10
    arrangements = {
        "inside one vector": lambda h, nv, t0: [h + 5 * vec + 1, h + 5 * vec + 2],
        "head and tail": lambda h, nv, t0: [0, V - 1],
        "two lanes of one wave": lambda h, nv, t0: [h + 3 * vec + 2, h + 10 * vec],
        "two waves": lambda h, nv, t0: [h + 7 * vec + 1, h + (7 + 64) * vec],
        "first and second vector of a thread": lambda h, nv, t0: [h + 9 * vec + 3, h + (9 + 256) * vec + 1],
    }
    base = _base_logits(N_ROWS, V, 77)
    tgt = torch.randint(0, V, (N_ROWS,), generator=torch.Generator().manual_seed(78))
    figures = {}
    for name, fn in arrangements.items():
        x = base.clone()
        first = []
        for n, (h, nv, t0) in enumerate(w):
            cols = fn(h, nv, t0)
            if three:
                cols = cols + [t0 - 1]                                    # a third one in the last vector
            x[n, cols] = 20.0                                             # exact in both dtypes
            first.append(min(cols))
        ref = run_and_judge(lib, Case(x, tgt, dtype, o, ld), f"ties {name} three={three} {dtype}", figures)
        assert ref["pred"].tolist() == first
    _print_figures(f"ties {dtype} three={three}", figures)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_ce_all_equal_row(lib, dtype):
    V = 2051
    x = torch.full((N_ROWS, V), 1.5)
    tgt = torch.arange(N_ROWS) * 200
    ref = run_and_judge(lib, Case(x, tgt, dtype, 1, V), f"all-equal {dtype}")
    assert torch.all(ref["pred"] == 0) and abs(float(ref["lse"][0]) - (1.5 + math.log(V))) < 1e-12


# ---------------------------------------------------------------------------------------------------------------
# c. range
# ---------------------------------------------------------------------------------------------------------------
def _range_rows(dtype, o, V):
    """Nine rows: +1e4 and -1e4 shifts, a spread of 80, one dominant logit at the target, and -inf logits off the target: a few
    scattered, everything thread 0 sees, a whole aligned vector a thread meets first, head and tail elements."""
    vec = 4 if dtype == F32 else 8
    w = walks(dtype, o, V, V)
    x = _base_logits(N_ROWS, V, 91)
    tgt = torch.randint(0, V, (N_ROWS,), generator=torch.Generator().manual_seed(92))
    x[0] += 1e4
    x[1] -= 1e4
    x[2] = torch.linspace(-80.0, 0.0, V)[torch.randperm(V, generator=torch.Generator().manual_seed(93))]
    x[3, tgt[3]] = 50.0
    ninf = [[] for _ in range(N_ROWS)]
    ninf[4] = [1, 17, 500, V - 2]
    h, nv, t0 = w[5]
    ninf[5] = ([0] if h else []) + [h + q * vec + u for q in range(0, nv, 256) for u in range(vec)] + ([t0] if t0 < V else [])
    h, nv, t0 = w[6]
    ninf[6] = [h + 9 * vec + u for u in range(vec)]                       # thread 9 has no head element: its first push
    h, nv, t0 = w[7]
    ninf[7] = list(range(h)) + list(range(t0, V)) + [h + 20 * vec, h + 20 * vec + vec - 1]
    for n in range(N_ROWS):
        cols = [c for c in ninf[n] if c != int(tgt[n])]
        x[n, cols] = -math.inf
        ninf[n] = cols
    return x, tgt, ninf


@pytest.mark.parametrize("o", [0, 1, 3])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_ce_range_and_minus_infinity(lib, dtype, o):
    """Non-target -inf logits are allowed (include/kvq.h): a finite lse, the same pred, gradient 0 on those columns."""
    V = 1027
    x, tgt, ninf = _range_rows(dtype, o, V)
    assert len(ninf[5]) >= 4 and len(ninf[6]) in (4, 8)
    figures = {}
    from kvq._ffi import check, stream_ptr
    case = Case(x, tgt, dtype, o, V)
    ref = run_and_judge(lib, case, f"range {dtype} o={o}", figures)
    assert abs(float(ref["grad"][3, tgt[3]])) < 1e-15                     # the dominant row: p ~ 1 at the target, the gradient cancels
    # gradient exactly 0 on the -inf columns
    dev = "cuda"
    t = tgt.to(dev)
    rl = torch.empty(N_ROWS, device=dev); lse = torch.empty(N_ROWS, device=dev); pred = torch.empty(N_ROWS, dtype=torch.int64, device=dev)
    check(lib.kvq_ce_forward(case.ptr(case.flat), t.data_ptr(), N_ROWS, V, V, case.io, rl.data_ptr(), lse.data_ptr(), pred.data_ptr(), None,
                             None, stream_ptr()), "fwd")
    g_flat = torch.full_like(case.flat, FRAME)
    check(lib.kvq_ce_backward(case.ptr(case.flat), t.data_ptr(), lse.data_ptr(), None, N_ROWS, V, V, case.io, case.ptr(g_flat), stream_ptr()), "bwd")
    g = case.rows(g_flat).cpu().float()
    for n in range(N_ROWS):
        assert torch.all(g[n, ninf[n]] == 0), f"row {n}: a -inf logit has a gradient"
    _print_figures(f"range {dtype} o={o}", figures)


# ---------------------------------------------------------------------------------------------------------------
# e. kvq_ce_forward_stats on constructed statistics
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_ce_forward_stats_on_built_statistics(lib, dtype, N):
    """The merge of per-tile statistics alone: V = 600 in tiles of 256 (the third one partial), a fourth tile wholly beyond V
    (-inf, 0, INT_MAX), a maximum tied across tiles 0 and 1 (the lower tile wins), tiles whose maximum is -inf (first and middle)."""
    from kvq import nnops
    V, ld, tiles = 600, 608, 4
    x = _base_logits(N, V, 300 + N)
    g = torch.Generator().manual_seed(301 + N)
    tgt = torch.randint(512, V, (N,), generator=g)                        # tile 2 stays finite in every row
    rows = torch.arange(N)
    a, b, c = rows[rows % 3 == 0], rows[rows % 3 == 1], rows[rows % 3 == 2]
    x[a, 40] = 20.0
    x[a, 300] = 20.0                                                      # the same maximum in tiles 0 and 1
    x[b, 256:512] = -math.inf
    x[c, 0:256] = -math.inf
    x = x.to(dtype)
    stats = R.ce_tile_stats(x.float(), V, tiles)
    assert torch.all(stats[:, 3, 0] == -math.inf) and torch.all(stats[b, 1, 0] == -math.inf) and torch.all(stats[c, 0, 0] == -math.inf)
    dev = "cuda"
    logits = torch.full((N, ld), FRAME, dtype=dtype)
    logits[:, :V] = x
    logits = logits.to(dev)
    rl = torch.empty(N, device=dev); lse = torch.empty(N, device=dev); pred = torch.empty(N + 1, dtype=torch.int64, device=dev)
    pred[N] = -5
    out = torch.empty(2, device=dev)
    nnops.ce_forward_stats(logits, tgt.to(dev), stats.to(dev), rl, lse, pred, out[0:], out[1:])
    ref = R.ce_ref(x.float(), tgt)
    assert int(pred[N]) == -5
    assert torch.equal(pred[:N].cpu(), ref["pred"]) and torch.all(ref["pred"][a] == 40)
    r_lse, r_loss = R.ce_row_ratio(lse, ref["lse"], ref), R.ce_row_ratio(rl, ref["row_loss"], ref)
    print(f"FIGURE ce stats {dtype} N={N}: worst ratios lse {float(r_lse.max()):.4f}, row_loss {float(r_loss.max()):.4f}")
    assert float(r_lse.max()) <= 1 and float(r_loss.max()) <= 1
    mean_ref = float(ref["row_loss"].mean())
    assert abs(out[0].item() - mean_ref) <= 1e-6 + 2e-6 * abs(mean_ref)
