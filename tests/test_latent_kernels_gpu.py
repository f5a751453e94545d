"""kvq_latent_group_sum / kvq_latent_shift / kvq_vq_lookup (csrc/kvq_latent.hip) against the torch f64 restatements of
tests/_latent_ref.py.

Shapes: B in {1, 6, 9, 70}, S = 12, H = 128, G = 3, f32 and bf16 -- one sentence; fewer sentences than a workgroup's run of 8; one
run and a second run of one; nine runs, i.e. nine slabs; plus H = 100 (f32: 16-byte pieces; bf16: rows of 200 bytes, every column
on its own), rows inside a wider tensor (row stride 160 > H, sentence stride above S * H; width 131: unaligned rows) and H = 102 in
rows of 104 (aligned rows whose last columns are no whole 16-byte piece).
Bounds: the table holds f64 sums of values that are exact in f64, added in another order than torch adds them: each addition is
within 2^-53 of its partial sum, so a cell is within (n - 1) * 2^-53 * sum|x| -- asserted as 1e-12 * sum|x| per cell (the bound
the issue sets).  Counts, shift and lookup are exact: compared bitwise."""
import functools

import pytest
import torch

import _latent_ref as R

pytestmark = pytest.mark.gpu

S, H, G = 12, 128, 3
DTYPES = [torch.float32, torch.bfloat16]


def _x(B, dtype, seed, h=H, pad=0):
    """[B, S, h] activations (a column slice of a [B, S, h + pad] tensor when pad > 0), labels in {-1, 0, 2}: group 1 stays empty"""
    g = torch.Generator().manual_seed(seed)
    full = (torch.randn(B, S, h + pad, generator=g) * 3).to(dtype).cuda()
    group = torch.tensor([(-1, 0, 2, 2, 0)[i % 5] for i in range(B)], dtype=torch.int32)
    if B == 1:
        group[0] = 2
    return (full[:, :, :h] if pad else full), group.cuda()


def _census(h=H):
    from kvq.census import LatentCensus
    return LatentCensus(G, S, h)


@functools.lru_cache(maxsize=None)
def filled(dtype):
    """a census over three batches (B = 6, 9, 70) and the same thing restated: shared by the shift tests, never written"""
    c = _census()
    xs = [_x(B, dtype, seed) for B, seed in ((6, 11), (9, 12), (70, 13))]
    for x, grp in xs:
        c.add(x, grp)
    table, count, mag, _ = R.group_sum_ref(torch.cat([x for x, _ in xs]), torch.cat([g for _, g in xs]), G)
    torch.cuda.synchronize()
    return c, table, count, mag


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,h,pad", [(1, H, 0), (6, H, 0), (9, H, 0), (70, H, 0), (9, 100, 0), (70, 100, 0), (9, H, 32), (9, H, 3), (9, 102, 2)])
def test_group_sum_equals_the_f64_sum(B, h, pad, dtype):
    x, grp = _x(B, dtype, 100 + B, h, pad)
    assert (x.stride(1) > h) == (pad > 0)
    c = _census(h)
    c.add(x, grp)
    table, count, mag, n_bad = R.group_sum_ref(x, grp, G)
    assert n_bad == 0 and torch.equal(c.count, count) and int(count[1]) == 0
    err = (c.table - table).abs()
    print(f"\n[group_sum] B={B} h={h} pad={pad} {dtype}: worst |table - f64 sum| / sum|x| = {float((err / mag.clamp(min=1e-300)).max()):.3e}")
    assert bool((err <= 1e-12 * mag).all())
    assert float(c.table[1].abs().max()) == 0.0                         # the group nobody belongs to
    res = c.results()
    assert res["count"].tolist() == count.tolist() and res["mean"].dtype == torch.float64 and not res["mean"].is_cuda
    want = table.cpu() / count.clamp(min=1).cpu().double().view(-1, 1, 1)
    assert float((res["mean"] - want).abs().max()) <= 1e-12 * float(mag.max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_three_adds_accumulate_and_skip_label_minus_one(dtype):
    c, table, count, mag = filled(dtype)
    assert torch.equal(c.count, count) and c.sentences == 85
    assert int(count.sum()) < 85 and int(count[1]) == 0                 # labels -1 were left out, group 1 stayed empty
    assert bool(((c.table - table).abs() <= 1e-12 * mag).all())
    assert torch.equal(c.direction(2, 0).cuda(), (c.results()["mean"][2] - c.results()["mean"][0]).cuda())


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_second_run_gives_identical_bits(dtype):
    c, _, _, _ = filled(dtype)
    again = _census()
    for B, seed in ((6, 11), (9, 12), (70, 13)):
        again.add(*_x(B, dtype, seed))
    assert torch.equal(again.table, c.table) and torch.equal(again.count, c.count)


def test_an_out_of_range_label_is_found_by_results():
    from kvq._ffi import KvqError
    x, grp = _x(9, torch.float32, 5)
    for bad in (G, -2):
        c = _census()
        g2 = grp.clone()
        g2[3] = bad
        c.add(x, g2)
        with pytest.raises(KvqError, match="group label"):
            c.results()
        keep = torch.ones(9, dtype=torch.bool)
        keep[3] = False
        table, count, _, _ = R.group_sum_ref(x[keep.cuda()], grp[keep.cuda()], G)
        assert torch.equal(c.count, count) and float((c.table - table).abs().max()) <= 1e-9       # the sentence was skipped
    with pytest.raises(KvqError, match="integer labels"):
        _census().add(x, torch.zeros(9).cuda())
    with pytest.raises(KvqError, match="latents must be"):
        _census().add(x[:, :5], 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,h,pad", [(1, H, 0), (9, H, 0), (70, H, 0), (9, 100, 0), (9, H, 32), (9, H, 3), (9, 102, 2)])
def test_shift_is_bitwise_the_restatement(B, h, pad, dtype):
    x, grp = _x(B, dtype, 200 + B, h, pad)
    if h == H:
        c, table, count, _ = filled(dtype)
    else:
        c = _census(h)
        big, gb = _x(70, dtype, 7, h)
        c.add(big, gb)
        table, count, _, _ = R.group_sum_ref(big, gb, G)
    g = torch.Generator().manual_seed(B)
    sel = (torch.rand(B, S, generator=g) < 0.6).cuda()
    for alpha, s in ((1.0, None), (-0.37, sel), (2.5, sel.to(torch.int8))):
        got = c.shift(x, 2, 0, alpha=alpha, sel=s)
        want = R.shift_ref(x, table, count, 2, 0, alpha=alpha, sel=s)
        assert got.dtype == dtype and got.is_contiguous() and torch.equal(got, want), (alpha, s is None)
        if s is not None:
            assert torch.equal(got[~sel], x[~sel])                      # unselected positions: the same bits
            assert not torch.equal(got[sel], x[sel])
    inplace = x.clone() if pad == 0 else x                              # (a slice: shifted where it lies, inside the wider tensor)
    before = inplace.clone()
    out = c.shift(inplace, 2, 0, alpha=-0.37, sel=sel, out=inplace)
    assert out is inplace and torch.equal(inplace, R.shift_ref(before, table, count, 2, 0, alpha=-0.37, sel=sel))


def test_shift_refuses_an_empty_group_and_the_kernel_leaves_the_rows_alone():
    from kvq import nnops
    from kvq._ffi import KvqError
    c, _, _, _ = filled(torch.float32)
    x, _ = _x(6, torch.float32, 3)
    for g1, g0 in ((1, 0), (2, 1)):
        with pytest.raises(KvqError, match="is empty"):
            c.shift(x, g1, g0)
        with pytest.raises(KvqError, match="is empty"):
            c.direction(g1, g0)
        assert torch.equal(nnops.latent_shift(x, c.table, c.count, g1, g0, 1.0), x)      # the library's own rule: no shift, no NaN
    with pytest.raises(KvqError, match="outside"):
        c.shift(x, 3, 0)
    with pytest.raises(KvqError, match="sel must be"):
        c.shift(x, 2, 0, sel=torch.ones(6, S + 1, dtype=torch.bool).cuda())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_factors,Dg", [(1, 128), (3, 128), (1, 100), (3, 100), (3, 36)])
def test_lookup_is_bitwise_the_codebook_rows(n_factors, Dg, dtype):
    from kvq import nnops
    K = 32
    g = torch.Generator().manual_seed(n_factors * 1000 + Dg)
    E = torch.randn(n_factors * K, Dg, generator=g).cuda()
    for N in (1, 70 * S):
        idx = torch.randint(0, K, (N, n_factors), generator=g).cuda()
        got = nnops.vq_lookup(idx, E, K, dtype)
        assert torch.equal(got, R.lookup_ref(E, idx, K, dtype))
        if n_factors == 1:
            assert torch.equal(got, E[idx[:, 0]].to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_lookup_counts_a_bad_index_and_leaves_a_zero_row(dtype):
    from kvq import nnops
    K, Dg = 32, 128
    E = torch.randn(3 * K, Dg, generator=torch.Generator().manual_seed(9)).cuda()
    idx = torch.randint(0, K, (20, 3), generator=torch.Generator().manual_seed(10)).cuda()
    idx[4, 1], idx[7, 2] = K, -1
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = nnops.vq_lookup(idx, E, K, dtype, n_bad=bad)
    assert int(bad.item()) == 2
    ok = idx.clamp(0, K - 1)
    want = R.lookup_ref(E, ok, K, dtype)
    want[4, Dg:2 * Dg] = 0
    want[7, 2 * Dg:] = 0
    assert torch.equal(got, want)
