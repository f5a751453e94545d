"""The kvq_*_ignore entry points of csrc/kvq_ce.hip (the reconstruction loss over the rows whose target differs from ignore_index;
DESIGN.md section 5g) against f64 from the up-cast logits (tests/_ce_ignore_ref.py), on the framed buffers and at the bounds of
tests/test_ce_parity_gpu.py: |lse - ref|, |row_loss - ref| <= 2^-20 M per counted row, the gradient within ce_grad_ratio <= 1 per
element, the mean loss within 1e-6 + 2e-6 |ref|, the accuracy within 1e-6 relative, the count exact.

Every case fills the logits of its ignored rows with NaN: an ignored row must not be read, so every output stays finite, its
row results are exactly (0, 0, ignore_index) and its gradient row -- padding columns included, in place and out of place -- is +0
by its bits.  With no row ignored every output has the bits of the entry point without ignore_index; with every row ignored
loss = acc = count = 0 and the whole gradient is 0.

A counted row's target must differ from ignore_index; where the vocabulary leaves no such id (V = 1 with ignore_index = 0 = V - 1)
every row is ignored whatever the pattern asks for, and the pattern "none" is not run."""
import math

import pytest
import torch

import _ce_ignore_ref as RI
import _pointwise_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
PAD = 64                      # frame elements around the logits (a multiple of 16 bytes in both dtypes)
FRAME = 3.0
N_ROWS = 9
N_TILED = 37                  # two row blocks of 32 of the tiled kernel, the second one short
G_LOSS = 1.7
VS = [1, 5, 13, 1027, 2 * 256 * 8 + 3]
PATTERNS = ["none", "all", "alternating", "first_block", "last_ignored", "last_counted"]


@pytest.fixture(scope="module")
def lib():
    from kvq import _ffi
    _ffi.lib()
    assert torch.cuda.is_available()
    return _ffi.lib()


class Case:
    """Logits x [N, V] (CPU, in `dtype`) placed in a flat framed buffer at storage offset o with row stride ld (as in
    tests/test_ce_parity_gpu.py)."""

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
        return torch.equal(bits(flat[:a]), bits(snap[:a])) and torch.equal(bits(flat[b:]), bits(snap[b:]))


def bits(t):
    """The words of t as integers: equality by bits, so NaN equals itself and -0 differs from +0."""
    t = t.detach().contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def ignored_rows(pattern, N):
    ign = torch.zeros(N, dtype=torch.bool)
    if pattern == "all":
        ign[:] = True
    elif pattern == "alternating":
        ign[::2] = True
    elif pattern == "first_block":          # the whole first 32-row block of the tiled kernel (all of a shorter batch)
        ign[:32] = True
    elif pattern == "last_ignored":         # the row the tiled kernel's clamped loads go to
        ign[N - 1] = True
    elif pattern == "last_counted":
        ign[:N - 1] = True
    else:
        assert pattern == "none"
    return ign


def make_case(pattern, N, V, ign_index, dtype, o, ld, seed):
    """(case, ignored [N] bool) or None when the pattern cannot be built: counted targets are drawn from [0, V) without
    ignore_index; ignored rows carry ignore_index as their target and NaN as their logits."""
    g = torch.Generator().manual_seed(seed)
    x = 2 * torch.randn(N, V, generator=g)
    allowed = torch.tensor([v for v in range(V) if v != ign_index][:4096] or [-1])
    ign = ignored_rows(pattern, N)
    if int(allowed[0]) < 0:                 # no id left for a counted row
        if pattern == "none":
            return None
        ign[:] = True
    tgt = allowed[torch.randint(0, len(allowed), (N,), generator=g)]
    tgt[~ign & (torch.arange(N) % 2 == 1)] = int(allowed[-1])              # (V - 1 where allowed: the last real column)
    tgt[ign] = ign_index
    x[ign] = math.nan
    return Case(x, tgt, dtype, o, ld), ign


def forward_ignore(lib, case, ign_index):
    from kvq._ffi import check, stream_ptr
    N, dev = case.N, "cuda"
    tgt = case.target.to(dev)
    rl = torch.full((N,), FRAME, device=dev); lse = torch.full((N,), FRAME, device=dev)
    pred = torch.full((N,), -7, dtype=torch.int64, device=dev)
    out = torch.full((3,), FRAME, device=dev)
    snap = case.flat.clone()
    check(lib.kvq_ce_forward_ignore(case.ptr(case.flat), tgt.data_ptr(), N, case.V, case.ld, case.io, ign_index, rl.data_ptr(),
                                    lse.data_ptr(), pred.data_ptr(), out[0:].data_ptr(), out[1:].data_ptr(), out[2:].data_ptr(),
                                    stream_ptr()), "kvq_ce_forward_ignore")
    assert torch.equal(bits(case.flat), bits(snap)), "the forward wrote to the logits"
    return tgt, rl, lse, pred, out


def judge_forward(what, case, ign, ign_index, rl, lse, pred, out, ref):
    for name, t in (("row_loss", rl), ("row_lse", lse), ("loss / acc / count", out)):
        assert torch.all(torch.isfinite(t)), f"{what}: {name} is not finite: {t.cpu().tolist()}"
    assert torch.equal(pred.cpu(), ref["pred"]), f"{what}: pred {pred.cpu().tolist()} != {ref['pred'].tolist()}"
    assert not bits(rl.cpu()[ign]).any() and not bits(lse.cpu()[ign]).any(), f"{what}: an ignored row's row_loss / row_lse is not +0"
    r_lse, r_loss = R.ce_row_ratio(lse, ref["lse"], ref), R.ce_row_ratio(rl, ref["row_loss"], ref)
    worst = dict(lse=float(r_lse.max()), row_loss=float(r_loss.max()))
    assert worst["lse"] <= 1 and worst["row_loss"] <= 1, f"{what}: lse / row_loss error over 2^-20 M: {worst}"
    loss, acc, count = (float(v) for v in out.cpu())
    assert count == ref["count"], f"{what}: count {count} != {ref['count']}"
    assert abs(loss - ref["loss"]) <= 1e-6 + 2e-6 * abs(ref["loss"]), f"{what}: mean loss {loss} vs {ref['loss']}"
    assert abs(acc - ref["acc"]) <= 1e-6 * ref["acc"], f"{what}: accuracy {acc} vs {ref['acc']}"
    if ref["count"] == 0:
        assert not bits(out.cpu()).any(), f"{what}: loss / acc / count of a batch without a counted row: {out.cpu().tolist()}"
    return worst


def judge_gradient(what, case, ign, g, ref):
    V = case.V
    assert torch.all(torch.isfinite(g.float())), f"{what}: the gradient is not finite"
    assert not bits(g[ign.to(g.device)]).any(), f"{what}: an ignored row of g_logits is not +0 everywhere (padding columns included)"
    assert torch.all(g[:, V:] == 0), f"{what}: padding columns are not zero"
    safe_t = torch.where(ign, torch.zeros_like(case.target), case.target)
    r_g = R.ce_grad_ratio(g[:, :V].cpu(), ref, case.dtype == BF16, safe_t)
    assert float(r_g.max()) <= 1, f"{what}: gradient error / tolerance {float(r_g.max()):.3f} at {divmod(int(r_g.argmax()), V)}"
    return float(r_g.max())


# ---------------------------------------------------------------------------------------------------------------
# the row kernels: kvq_ce_forward_ignore, kvq_ce_backward_ignore
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("o", [0, 1, 3])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_row_kernels(lib, dtype, o, pattern):
    from kvq._ffi import check, stream_ptr
    dev = "cuda"
    figures, ran = {}, 0
    for V in VS:
        for ld in sorted({V, V + 3}):
            for ign_index in sorted({0, V - 1, -100}):
                made = make_case(pattern, N_ROWS, V, ign_index, dtype, o, ld, seed=1000 * V + 7 * o + (ign_index % 5))
                if made is None:
                    continue
                case, ign = made
                what = f"{pattern} V={V} ld={ld} o={o} {dtype} ignore_index={ign_index}"
                N = case.N
                tgt, rl, lse, pred, out = forward_ignore(lib, case, ign_index)
                ref = RI.ce_ignore_ref(case.x.float(), case.target, ign_index, G_LOSS)
                assert ref["count"] == int((~ign).sum())
                w = judge_forward(what, case, ign, ign_index, rl, lse, pred, out, ref)
                gs = torch.full((1,), G_LOSS, device=dev)
                snap = case.flat.clone()
                g_flat = torch.full_like(case.flat, FRAME)
                g_snap = g_flat.clone()
                check(lib.kvq_ce_backward_ignore(case.ptr(case.flat), tgt.data_ptr(), lse.data_ptr(), gs.data_ptr(), out[2:].data_ptr(),
                                                 ign_index, N, V, ld, case.io, case.ptr(g_flat), stream_ptr()), "kvq_ce_backward_ignore")
                in_flat = case.flat.clone()
                check(lib.kvq_ce_backward_ignore(case.ptr(in_flat), tgt.data_ptr(), lse.data_ptr(), gs.data_ptr(), out[2:].data_ptr(),
                                                 ign_index, N, V, ld, case.io, case.ptr(in_flat), stream_ptr()), "kvq_ce_backward_ignore in place")
                assert torch.equal(bits(case.flat), bits(snap)), f"{what}: the out-of-place backward wrote to the logits"
                assert case.outside_untouched(g_flat, g_snap) and case.outside_untouched(in_flat, snap), f"{what}: wrote outside the view"
                g = case.rows(g_flat)
                assert torch.equal(bits(g), bits(case.rows(in_flat))), f"{what}: in-place and out-of-place gradients differ"
                w["grad"] = judge_gradient(what, case, ign, g, ref)
                if pattern == "all" or ref["count"] == 0:
                    assert not bits(g).any(), f"{what}: the gradient of a batch without a counted row is not 0"
                if pattern == "none":
                    # bit for bit the entry points without ignore_index
                    rl0 = torch.empty_like(rl); lse0 = torch.empty_like(lse); pred0 = torch.empty_like(pred); out0 = torch.empty(2, device=dev)
                    check(lib.kvq_ce_forward(case.ptr(case.flat), tgt.data_ptr(), N, V, ld, case.io, rl0.data_ptr(), lse0.data_ptr(),
                                             pred0.data_ptr(), out0[0:].data_ptr(), out0[1:].data_ptr(), stream_ptr()), "kvq_ce_forward")
                    g0_flat = torch.full_like(case.flat, FRAME)
                    check(lib.kvq_ce_backward(case.ptr(case.flat), tgt.data_ptr(), lse0.data_ptr(), gs.data_ptr(), N, V, ld, case.io,
                                              case.ptr(g0_flat), stream_ptr()), "kvq_ce_backward")
                    for name, a, b in (("row_loss", rl, rl0), ("row_lse", lse, lse0), ("pred", pred, pred0), ("loss, acc", out[:2], out0),
                                       ("g_logits", g_flat, g0_flat)):
                        assert torch.equal(bits(a), bits(b)), f"{what}: {name} differs from the entry point without ignore_index"
                    assert float(out[2]) == N
                for k, v in w.items():
                    figures[k] = max(figures.get(k, 0.0), v)
                ran += 1
    assert ran == (26 if pattern == "none" else 28)
    print(f"FIGURE ce_ignore rows {pattern} {dtype} o={o}: {ran} cases, worst ratios " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(figures.items())))


# ---------------------------------------------------------------------------------------------------------------
# the tiled kernel: kvq_ce_backward_bias_ignore
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_tiled_backward_with_bias_partials(lib, dtype, pattern):
    from kvq._ffi import check, stream_ptr
    dev = "cuda"
    N = N_TILED
    P = lib.kvq_ce_bwd_partial_rows(N)
    assert P == 2
    worst, ran = 0.0, 0
    for V in VS:
        ld = (V + 7) // 8 * 8
        assert ld > V and ld % 8 == 0
        for ign_index in sorted({0, V - 1, -100}):
            made = make_case(pattern, N, V, ign_index, dtype, 0, ld, seed=2000 * V + (ign_index % 5))
            if made is None:
                continue
            case, ign = made
            what = f"tiled {pattern} V={V} {dtype} ignore_index={ign_index}"
            tgt, rl, lse, pred, out = forward_ignore(lib, case, ign_index)
            ref = RI.ce_ignore_ref(case.x.float(), case.target, ign_index, G_LOSS)
            judge_forward(what, case, ign, ign_index, rl, lse, pred, out, ref)
            gs = torch.full((1,), G_LOSS, device=dev)
            snap = case.flat.clone()
            results = []
            for in_place in (False, True):
                g_flat = case.flat.clone() if in_place else torch.full_like(case.flat, FRAME)
                g_snap = g_flat.clone()
                part = torch.full((PAD + P * ld + PAD,), FRAME, device=dev)
                check(lib.kvq_ce_backward_bias_ignore(case.ptr(g_flat if in_place else case.flat), tgt.data_ptr(), lse.data_ptr(),
                                                      gs.data_ptr(), out[2:].data_ptr(), ign_index, N, V, ld, case.io, case.ptr(g_flat),
                                                      part[PAD:].data_ptr(), P * ld * 4, stream_ptr()), "kvq_ce_backward_bias_ignore")
                assert torch.equal(bits(case.flat), bits(snap)), f"{what}: the logits of the out-of-place call changed"
                assert case.outside_untouched(g_flat, g_snap) and torch.all(part[:PAD] == FRAME) and torch.all(part[PAD + P * ld:] == FRAME), \
                    f"{what}: wrote outside the view"
                results.append((g_flat, part))
            (g_flat, part), (g_in, part_in) = results
            assert torch.equal(bits(g_flat), bits(g_in)) and torch.equal(bits(part), bits(part_in)), f"{what}: in place differs from out of place"
            g = case.rows(g_flat)
            pr = part[PAD:PAD + P * ld].view(P, ld)
            assert torch.all(torch.isfinite(pr)), f"{what}: a bias partial is not finite"
            assert torch.all(pr[:, V:] == 0), f"{what}: padding columns of the partials are not zero"
            worst = max(worst, judge_gradient(what, case, ign, g, ref))
            st = g[:, :V].cpu().double()
            for p in range(P):
                blk = st[p * 32:(p + 1) * 32]                                 # ignored rows are stored zeros: they add 0
                bound = 31 * 2.0 ** -24 * blk.abs().sum(0)                    # at most 31 f32 additions of the stored values
                assert torch.all((pr[p, :V].cpu().double() - blk.sum(0)).abs() <= bound), f"{what}: partial row {p} is not the f32 sum of the stored values"
                if bool(ign[p * 32:(p + 1) * 32].all()):
                    assert not bits(pr[p]).any(), f"{what}: the partial row of a block of ignored rows is not +0"
            if pattern == "all" or ref["count"] == 0:
                assert not bits(g).any() and not bits(pr).any(), f"{what}: gradient / partials of a batch without a counted row are not 0"
            if pattern == "none":
                g0_flat = torch.full_like(case.flat, FRAME)
                part0 = torch.full_like(part, FRAME)
                check(lib.kvq_ce_backward_bias(case.ptr(case.flat), tgt.data_ptr(), lse.data_ptr(), gs.data_ptr(), N, V, ld, case.io,
                                               case.ptr(g0_flat), part0[PAD:].data_ptr(), P * ld * 4, stream_ptr()), "kvq_ce_backward_bias")
                assert torch.equal(bits(g_flat), bits(g0_flat)), f"{what}: g_logits differs from kvq_ce_backward_bias"
                assert torch.equal(bits(part), bits(part0)), f"{what}: the bias partials differ from kvq_ce_backward_bias"
            ran += 1
    assert ran == (13 if pattern == "none" else 14)
    print(f"FIGURE ce_ignore tiled {pattern} {dtype}: {ran} cases, worst gradient ratio {worst:.4f}")


# ---------------------------------------------------------------------------------------------------------------
# kvq_seq_acc_ignore
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ign_index", [0, -100, 29])
@pytest.mark.parametrize("S", [1, 12, 32, 70])
def test_sentence_accuracy_over_counted_tokens(lib, S, ign_index):
    from kvq._ffi import check, stream_ptr
    B = 5
    g = torch.Generator().manual_seed(S)
    tgt = torch.randint(1, 29, (B, S), generator=g)
    pred = torch.where(torch.rand(B, S, generator=g) < 0.6, tgt, torch.randint(1, 29, (B, S), generator=g))
    n_real = [S, max(S // 3, 1), 0, max(S - 1, 1), (S + 1) // 2]          # sentence 2 has no counted token
    for b, n in enumerate(n_real):
        tgt[b, n:] = ign_index
        pred[b, n:] = ign_index                                           # what the forward writes there: must not count as a hit
    want = RI.seq_acc_ignore_ref(pred, tgt, ign_index)
    assert float(want[2]) == 0.0 and float(want.max()) > 0
    out = torch.full((B + 1,), FRAME, device="cuda")
    pred_d, tgt_d = pred.cuda(), tgt.cuda()
    check(lib.kvq_seq_acc_ignore(pred_d.data_ptr(), tgt_d.data_ptr(), B, S, ign_index, out.data_ptr(), stream_ptr()),
          "kvq_seq_acc_ignore")
    assert float(out[B]) == FRAME
    assert torch.equal(bits(out[:B].cpu()), bits(want)), f"S={S}: {out[:B].cpu().tolist()} != {want.tolist()}"


# ---------------------------------------------------------------------------------------------------------------
# kvq_ce_forward_stats_ignore on constructed statistics
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ign_index", [-100, 0])
@pytest.mark.parametrize("N", [1, 257])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_forward_from_built_statistics(lib, dtype, N, ign_index):
    """The statistics of tests/test_ce_parity_gpu.py::test_ce_forward_stats_on_built_statistics (V = 600 in tiles of 256, a tile
    beyond V, a maximum tied across tiles, tiles whose maximum is -inf) with every third row ignored -- row 0 first, so N = 1 is a
    batch without a counted row; the statistics and the logits of the ignored rows are NaN."""
    from kvq import nnops
    V, ld, tiles = 600, 608, 4
    g = torch.Generator().manual_seed(300 + N)
    x = 2 * torch.randn(N, V, generator=g)
    tgt = torch.randint(512, V, (N,), generator=g)                        # tile 2 stays finite in every row
    rows = torch.arange(N)
    a, b, c = rows[rows % 3 == 0], rows[rows % 3 == 1], rows[rows % 3 == 2]
    x[a, 40] = 20.0
    x[a, 300] = 20.0
    x[b, 256:512] = -math.inf
    x[c, 0:256] = -math.inf
    x = x.to(dtype)
    ign = (rows % 6 == 0) | (rows % 6 == 4) if N > 1 else torch.ones(1, dtype=torch.bool)      # every third row, of kinds a and b
    assert N == 1 or abs(int(ign.sum()) - N // 3) <= 1
    stats = R.ce_tile_stats(x.float(), V, tiles)
    tgt[ign] = ign_index
    x[ign] = math.nan
    stats[ign] = math.nan
    dev = "cuda"
    logits = torch.full((N, ld), FRAME, dtype=dtype)
    logits[:, :V] = x
    logits = logits.to(dev)
    snap = logits.clone()
    rl = torch.full((N,), FRAME, device=dev); lse = torch.full((N,), FRAME, device=dev)
    pred = torch.full((N + 1,), -5, dtype=torch.int64, device=dev)
    out = torch.full((3,), FRAME, device=dev)
    tgt_d, stats_d = tgt.to(dev), stats.to(dev)
    nnops.ce_forward_stats(logits, tgt_d, stats_d, rl, lse, pred, out[0:], out[1:], ignore_index=ign_index, count=out[2:])
    assert torch.equal(bits(logits), bits(snap)) and int(pred[N]) == -5
    ref = RI.ce_ignore_ref(x.float(), tgt, ign_index)
    w = judge_forward(f"stats N={N} {dtype}", None, ign, ign_index, rl, lse, pred[:N], out, ref)
    print(f"FIGURE ce_ignore stats {dtype} N={N}: count {ref['count']}, worst ratios lse {w['lse']:.4f}, row_loss {w['row_loss']:.4f}")
    if N > 1:
        keep = a[~ign[a]]
        assert len(keep) and torch.all(ref["pred"][keep] == 40)
