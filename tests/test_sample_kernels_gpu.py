"""kvq_gen_select_filtered (csrc/kvq_generate.hip) against the f64 reference of tests/_sample_ref.py and against kvq_gen_select itself.

Exact where the contract is exact: with the filters off the bits of kvq_gen_select; under top-k the size of the kept set and its
last element, ties included; the kept set a prefix of the order, always; the choice = kvq_gen_select on the logits with everything
outside the kept set at -inf.  Under top-p the size of the kept set must lie in keep_band(TOL_MASS) -- the exact answers at
top_p -+ 2^-17, the bound derived from the kernel's summation order (include/kvq.h) -- and the score of the choice within the derived
bound of the f64 value.  Every output sits between guard words.

Rows of a case (the pool): 0 N(0, 1); 1 every logit equal; 2 sixteen distinct values (every cut falls inside a tied group);
3 N(0, 3) with NaN and -inf columns; 4 N(0, 3); 5 N(0, 6); 6 N(0, 1) rounded to bf16 (tens of ties at any cut).  B = 7 runs the pool,
B = 1 its rows 2 and 1 alone.  Columns V .. ld-1 hold 1e30: they must never count.
"""
import pytest
import torch

import _gen_ref as R
import _sample_ref as S

pytestmark = pytest.mark.gpu

GUARD = 64
DTYPES = [torch.bfloat16, torch.float32]
SHAPES = [(5, 8), (37, 40), (2048, 2048), (30522, 30528)]
LMAX = 4
NAN, NINF = float("nan"), float("-inf")


def framed(shape, dtype, fill):
    """(whole, view): `view` of the given shape inside a flat buffer with GUARD sentinel elements on both sides"""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), -7.0 if dtype.is_floating_point else -7, dtype=dtype, device="cuda")
    view = whole[GUARD:GUARD + n].view(*shape)
    view.fill_(fill)
    return whole, view


def guards_intact(whole):
    return bool((whole[:GUARD] == -7).all()) and bool((whole[-GUARD:] == -7).all())


def state(t, P=1, Lmax=LMAX, eos=None, pad=0, tau=0.0, seed=0):
    from kvq import nnops
    return nnops.new_gen_state("cuda", t, P, Lmax, eos, pad, temperature=tau, seed=seed)


@pytest.fixture(scope="module")
def pools():
    """the pool of every (V, ld), built once and left unchanged"""
    out = {}
    for V, ld in SHAPES:
        g = torch.Generator().manual_seed(V)
        x = torch.full((7, ld), 1e30)
        x[0, :V] = torch.randn(V, generator=g)
        x[1, :V] = 0.25
        x[2, :V] = torch.linspace(-3.0, 3.0, 16)[torch.randint(0, 16, (V,), generator=g)]
        x[3, :V] = 3.0 * torch.randn(V, generator=g)
        x[3, 0] = x[3, V // 3] = NAN
        x[3, V - 1] = NINF
        x[4, :V] = 3.0 * torch.randn(V, generator=g)
        x[5, :V] = 6.0 * torch.randn(V, generator=g)
        x[6, :V] = torch.randn(V, generator=g).bfloat16().float()
        out[V] = x
    return out


def rows_of(pools, V, B):
    return [pools[V]] if B == 7 else [pools[V][2:3], pools[V][1:2]]


class Launch:
    """one launch of kvq_gen_select_filtered on host rows x [B, ld]; every buffer framed by guard words"""

    def __init__(self, x, V, dtype, tau=1.0, seed=0, t=1, k=0, p=1.0, filt=None, want_logits=False, st=None):
        from kvq import nnops
        B, ld = x.shape
        self.V, self.t, self.tau = V, t, tau
        self.frames = []

        def buf(shape, dt, fill):
            whole, view = framed(shape, dt, fill)
            self.frames.append(whole)
            return view

        self.logits = buf((B, ld), dtype, 0)
        self.logits.copy_(x.to(dtype))
        self.ids, self.fin, self.lens = buf((B, LMAX), torch.int64, 9), buf((B,), torch.int32, 0), buf((B,), torch.int32, LMAX)
        self.kept_buf, self.cut_buf, self.lp_buf = buf((B, LMAX), torch.int32, -3), buf((B, LMAX), torch.int32, -3), buf((B, LMAX), torch.float32, -3.0)
        self.step_logits = buf((B, LMAX, V), torch.float32, 0.0) if want_logits else None
        self.st = state(t, tau=tau, seed=seed) if st is None else st
        self.filt = nnops.new_gen_filter("cuda", k, p) if filt is None else filt
        self.go()

    def go(self):
        from kvq import nnops
        nnops.gen_select_filtered(self.st, self.filt, self.logits, self.V, self.ids, self.fin, self.lens, self.step_logits, self.kept_buf,
                                  self.cut_buf, self.lp_buf)
        torch.cuda.synchronize()
        t = self.t
        assert all(guards_intact(w) for w in self.frames)
        other = [c for c in range(LMAX) if c != t]
        assert bool((self.kept_buf[:, other] == -3).all()) and bool((self.cut_buf[:, other] == -3).all()) and bool((self.lp_buf[:, other] == -3).all())
        self.choice = self.ids[:, t + 1].cpu() if t + 1 < LMAX else None
        self.kept, self.cut, self.lp = self.kept_buf[:, t].cpu().long(), self.cut_buf[:, t].cpu().long(), self.lp_buf[:, t].cpu()
        self.seen = self.logits[:, :self.V].float().cpu()
        self.y = S.y_of(self.seen, self.tau)
        return self

    def plain_choice(self, logits=None):
        """kvq_gen_select with the same state on the same (or the given) logits"""
        from kvq import nnops
        B = self.logits.shape[0]
        ids = torch.full((B, LMAX), 9, dtype=torch.int64, device="cuda")
        fin, lens = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.full((B,), LMAX, dtype=torch.int32, device="cuda")
        sl = None if self.step_logits is None else torch.zeros_like(self.step_logits)
        nnops.gen_select(self.st, self.logits if logits is None else logits, self.V, ids, fin, lens, sl)
        torch.cuda.synchronize()
        return ids.cpu(), fin.cpu(), lens.cpu(), None if sl is None else sl.cpu()


def prefix_check(run, ref):
    """the kept set is a prefix of the reference order: rank(cut) + 1 == kept, exactly, ties included"""
    some = run.kept > 0
    rank = ref.rank.gather(1, run.cut.clamp(min=0).unsqueeze(1)).squeeze(1)
    assert torch.equal((rank + 1)[some], run.kept[some]), (rank + 1, run.kept)
    assert bool((run.cut[~some] == -1).all())


CASES = pytest.mark.parametrize("V,ld,B,dtype", [(V, ld, B, dt) for V, ld in SHAPES for B in (1, 7) for dt in DTYPES])


# ---------------------------------------------------------------------------------------------------------------- 1 filters off
@CASES
def test_filters_off_has_the_bits_of_gen_select(pools, V, ld, B, dtype):
    for x in rows_of(pools, V, B):
        for tau, seed in ((0.7, 11), (0.0, 0)):
            run = Launch(x, V, dtype, tau=tau, seed=seed, want_logits=True)
            ids, fin, lens, sl = run.plain_choice()
            assert torch.equal(run.ids.cpu(), ids) and torch.equal(run.fin.cpu(), fin) and torch.equal(run.lens.cpu(), lens)
            assert torch.equal(torch.nan_to_num(run.step_logits.cpu(), nan=123.0), torch.nan_to_num(sl, nan=123.0))
            ref = S.Cut(run.y, 0, 1.0)
            assert torch.equal(run.kept, ref.n_valid) and torch.equal(run.cut, ref.cut)


# ---------------------------------------------------------------------------------------------------------------- 2 top-k
@CASES
def test_top_k_keeps_exactly_the_first_k_of_the_order(pools, V, ld, B, dtype):
    for x in rows_of(pools, V, B):
        for k in sorted({1, 2, 50, V - 1, V, V + 5}):
            run = Launch(x, V, dtype, tau=0.7, seed=k, k=k)
            ref = S.Cut(run.y, k, 1.0)
            assert torch.equal(run.kept, torch.clamp(ref.n_valid, max=k)) and torch.equal(run.kept, ref.n_keep)
            assert torch.equal(run.cut, ref.cut), (k, run.cut, ref.cut)
            if x.shape[0] == 1 and k <= V and bool((run.seen == run.seen[0, 0]).all()):
                assert int(run.cut[0]) == k - 1                              # every logit equal: ids 0 .. k - 1


# ---------------------------------------------------------------------------------------------------------------- 3 top-p
@CASES
def test_top_p_keeps_a_prefix_whose_size_lies_in_the_derived_band(pools, V, ld, B, dtype):
    widths = []
    for x in rows_of(pools, V, B):
        for p in (2.0 ** -20, 0.3, 0.5, 0.9, 0.95, 1.0 - 2.0 ** -20):
            run = Launch(x, V, dtype, tau=1.0, seed=3, p=p)
            ref = S.Cut(run.y, 0, p)
            prefix_check(run, ref)
            lo, hi = ref.keep_band(S.TOL_MASS)
            widths.append((p, run.kept.tolist(), (hi - lo).tolist()))
            assert bool((lo <= run.kept).all()) and bool((run.kept <= hi).all()), (p, lo, run.kept, hi)
    print(f"\n[top-p V={V} B={B} {dtype}] (p, kept, band width): " + "; ".join(f"{p:.6g} {k} {w}" for p, k, w in widths))


def test_top_p_with_a_tied_group_straddling_p():
    """one token of mass 1/2, then 20 tied tokens of mass 1/40 each: p = 0.7 is crossed by the 8th of them (1/2 + 8/40 = 0.7 exactly
    only in exact arithmetic: the band says 8 or 9), p = 0.74 by the 10th; the cut is the lowest indices of the group"""
    import math
    V = 64
    x = torch.full((1, V), -60.0)
    tied = list(range(40, 60))
    x[0, 7] = math.log(20.0)
    x[0, tied] = 0.0
    for dtype in DTYPES:
        for p, want in ((0.74, 11), (0.62, 6), (0.5 - 2.0 ** -10, 1), (0.99, 21)):
            run = Launch(x, V, dtype, tau=1.0, seed=1, p=p)
            ref = S.Cut(run.y, 0, p)
            lo, hi = ref.keep_band()
            prefix_check(run, ref)
            assert int(lo[0]) <= int(run.kept[0]) <= int(hi[0])
            if dtype == torch.float32:
                assert int(lo[0]) == int(hi[0]) == want == int(run.kept[0])
                assert int(run.cut[0]) == (7 if want == 1 else tied[want - 2])
        run = Launch(x, V, dtype, tau=1.0, seed=1, p=0.7)
        lo, hi = S.Cut(run.y, 0, 0.7).keep_band()
        assert int(lo[0]) <= int(run.kept[0]) <= int(hi[0]) and int(run.kept[0]) in (9, 10)


# ---------------------------------------------------------------------------------------------------------------- 4 k and p together
@CASES
def test_top_p_is_taken_inside_top_k_renormalised(pools, V, ld, B, dtype):
    x = torch.full((B, ld), 1e30)
    x[:, :V] = -30.0
    x[:, V - 4:V] = 2.0                                                      # four equal tokens hold the mass
    alone = Launch(x, V, dtype, tau=1.0, p=0.6)
    both = Launch(x, V, dtype, tau=1.0, k=2, p=0.6)
    for run, k, want in ((alone, 0, 3), (both, 2, 2)):
        ref = S.Cut(run.y, k, 0.6)
        lo, hi = ref.keep_band()
        assert torch.equal(lo, hi) and bool((run.kept == want).all()) and torch.equal(run.kept, ref.n_keep)
        assert bool((run.cut == V - 4 + want - 1).all())
    if B == 7:                                                               # and on the pool, against the band
        for k, p in ((50, 0.9), (2, 0.5), (V - 1, 0.3)):
            run = Launch(pools[V], V, dtype, tau=0.7, seed=2, k=k, p=p)
            ref = S.Cut(run.y, k, p)
            prefix_check(run, ref)
            lo, hi = ref.keep_band()
            assert bool((lo <= run.kept).all()) and bool((run.kept <= hi).all()) and bool((run.kept <= k).all())


# ---------------------------------------------------------------------------------------------------------------- 5 choice, 7 score
@CASES
def test_choice_is_gen_select_on_the_masked_logits_and_its_score_is_within_the_bound(pools, V, ld, B, dtype):
    worst = 0.0
    for x in rows_of(pools, V, B):
        for seed, t, k, p, tau in ((1, 0, 50, 1.0, 1.0), (2, 1, 0, 0.9, 0.7), (1 << 40, 2, 7, 0.5, 1.3), (3, 1, 0, 1.0, 1.0)):
            run = Launch(x, V, dtype, tau=tau, seed=seed, t=t, k=k, p=p)
            ref = S.Cut(run.y, k, p)
            prefix_check(run, ref)
            kept = ref.kept(run.kept)                                        # rebuilt from the kernel's own (kept, cut) by the order
            masked = run.logits.clone()
            masked[:, :V] = S.masked_logits(run.logits[:, :V], kept)
            want = run.plain_choice(masked)[0][:, t + 1]
            assert torch.equal(run.choice, want)
            some = run.kept > 0
            assert bool(kept.gather(1, run.choice.unsqueeze(1)).squeeze(1)[some].all())
            lp, bound = ref.logprob(run.choice, run.kept.clamp(min=1))
            err = (run.lp.double() - lp).abs()
            ok = some & lp.isfinite()
            assert bool(ok.any())
            worst = max(worst, float((err[ok] / bound[ok]).max()))
            assert bool((err[ok] <= bound[ok]).all()), (err, bound)
    print(f"\n[filtered score V={V} B={B} {dtype}] worst |step_logprob - f64| / bound = {worst:.3f}")


# ---------------------------------------------------------------------------------------------------------------- 6 distribution
@pytest.mark.parametrize("k,p", [(3, 1.0), (0, 0.7), (3, 0.7)])
def test_draws_follow_the_renormalised_distribution_and_stay_inside_the_set(k, p):
    from kvq import nnops
    N, V = 8192, 8
    row = torch.tensor([0.0, 1.0, -1.0, 2.0, 0.5, -2.0, 1.5, 0.25])
    logits = row.repeat(N, 1).cuda()
    ref = S.Cut(S.y_of(row.unsqueeze(0), 1.0), k, p)
    prob = ref.probs()[0]
    ids = torch.zeros((N, LMAX), dtype=torch.int64, device="cuda")
    fin, lens = torch.zeros(N, dtype=torch.int32, device="cuda"), torch.full((N,), LMAX, dtype=torch.int32, device="cuda")
    kept = torch.zeros((N, LMAX), dtype=torch.int32, device="cuda")
    st, filt = state(0), nnops.new_gen_filter("cuda", k, p)

    def draw(t, seed):
        st.copy_(state(t, tau=1.0, seed=seed))
        nnops.gen_select_filtered(st, filt, logits, V, ids, fin, lens, None, kept, None, None)
        return ids[:, t + 1].cpu()

    a = draw(0, 1234)
    assert bool((kept[:, 0] == int(ref.n_keep[0])).all())
    freq = torch.bincount(a, minlength=V).double() / N
    inside = prob > 0
    assert float(freq[~inside].sum()) == 0.0                                 # no draw falls outside the set
    dev = (freq - prob).abs()[inside] / R.frequency_bound(prob, N)[inside]
    print(f"\n[filtered sampling k={k} p={p}] kept {int(ref.n_keep[0])}, frequency deviation / (5 sigma): " + ", ".join(f"{d:.3f}" for d in dev.tolist()))
    assert bool((dev <= 1.0).all())
    assert torch.equal(a, draw(0, 1234))
    assert not torch.equal(a, draw(1, 1234)) and not torch.equal(a, draw(0, 1235))


# ---------------------------------------------------------------------------------------------------------------- 8 NaN, -inf, greedy
@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_minus_inf_columns_a_row_of_nans_and_a_greedy_state(dtype):
    V, ld = 37, 40
    g = torch.Generator().manual_seed(8)
    x = torch.full((4, ld), 1e30)
    x[:, :V] = torch.randn((4, V), generator=g)
    x[0, [0, 5, 36]] = NAN
    x[0, [1, 6]] = NINF
    x[1, :V] = NAN                                                           # a row with no valid logit
    x[2, :V] = NINF
    x[2, 9] = 0.5                                                            # a single token with mass
    for k, p in ((0, 1.0), (4, 1.0), (0, 0.8), (40, 0.999)):
        run = Launch(x, V, dtype, tau=0.9, seed=5, k=k, p=p)
        ref = S.Cut(run.y[[0, 2, 3]], k, p)
        got_kept, got_cut = run.kept[[0, 2, 3]], run.cut[[0, 2, 3]]
        lo, hi = ref.keep_band()
        assert bool((lo <= got_kept).all()) and bool((got_kept <= hi).all())
        if p == 1.0:
            assert torch.equal(got_kept, ref.n_keep) and torch.equal(got_cut, ref.cut)
        assert int(run.choice[1]) == 0 and int(run.kept[1]) == 0 and int(run.cut[1]) == -1 and bool(run.lp[1].isnan())
        assert int(run.choice[2]) == 9 and (p == 1.0 or int(run.kept[2]) == 1)
        assert not bool(run.y[0, run.choice[0]].isnan())
    # a greedy state ignores the filters: the arg-max, kept = n_valid, the score under the full softmax
    run = Launch(x, V, dtype, tau=0.0, seed=5, k=2, p=0.3)
    seen = torch.where(run.seen.isnan(), torch.full_like(run.seen, NINF), run.seen)
    assert run.choice.tolist() == seen.argmax(1).tolist()
    assert run.kept.tolist() == (~run.seen.isnan()).sum(1).tolist()
    ref = S.Cut(run.y[[0, 3]], 0, 1.0, greedy=True)
    lp, bound = ref.logprob(run.choice[[0, 3]])
    assert bool(((run.lp[[0, 3]].double() - lp).abs() <= bound).all())


# ---------------------------------------------------------------------------------------------------------------- 9 state on the device
def test_filters_are_read_from_the_device_state_and_a_reserved_word_stores_nothing(pools):
    from kvq import nnops
    V = 2048
    run = Launch(pools[V], V, torch.float32, tau=1.0, seed=4, k=5)
    assert run.kept.tolist() == [5] * 7
    for k, p in ((0, 0.5), (17, 1.0), (17, 0.25)):
        run.filt.copy_(torch.tensor(nnops.gen_filter_words(k, p), dtype=torch.int32))      # the SAME launch arguments
        run.go()
        ref = S.Cut(run.y, k, p)
        lo, hi = ref.keep_band()
        assert bool((lo <= run.kept).all()) and bool((run.kept <= hi).all())
    before = [w.clone() for w in run.frames]
    for word in (2, 3):
        words = nnops.gen_filter_words(5, 1.0)
        words[word] = 1
        run.filt.copy_(torch.tensor(words, dtype=torch.int32))
        run.ids.fill_(9)
        run.kept_buf.fill_(-3)
        nnops.gen_select_filtered(run.st, run.filt, run.logits, V, run.ids, run.fin, run.lens, None, run.kept_buf, run.cut_buf, run.lp_buf)
        torch.cuda.synchronize()
        assert bool((run.ids == 9).all()) and bool((run.kept_buf == -3).all()) and not bool(run.fin.any())
    assert len(before) == len(run.frames) and all(guards_intact(w) for w in run.frames)


# ---------------------------------------------------------------------------------------------------------------- 10 bookkeeping
@pytest.mark.parametrize("eos", [5, None])
def test_bookkeeping_is_gen_selects_prompt_end_token_and_pads(eos):
    from kvq import nnops
    B, V, Lmax, P, pad = 4, 16, 8, 3, 0
    frames = []

    def buf(shape, dt, fill):
        whole, view = framed(shape, dt, fill)
        frames.append(whole)
        return view

    ids, fin, lens = buf((B, Lmax), torch.int64, pad), buf((B,), torch.int32, 0), buf((B,), torch.int32, Lmax)
    kept, cut, lp = buf((B, Lmax), torch.int32, -3), buf((B, Lmax), torch.int32, -3), buf((B, Lmax), torch.float32, -3.0)
    prompt = torch.tensor([[11, 12, 13]] * B)
    ids[:, :P] = prompt.cuda()
    plan = torch.tensor([[(3 * t + b) % 4 + 6 for t in range(Lmax - 1)] for b in range(B)])
    plan[1, 3], plan[2, 6] = 5, 5
    plan[:, :2] = 5
    st = state(0, P=P, Lmax=Lmax, eos=eos, pad=pad, tau=1.0, seed=9)
    filt = nnops.new_gen_filter("cuda", 1, 1.0)                              # top_k = 1 under sampling: the planned token, whatever the noise
    h_ids, h_fin, h_len = ids.cpu().clone(), torch.zeros(B, dtype=torch.int32), torch.full((B,), Lmax, dtype=torch.int32)
    for t in range(Lmax - 1):
        logits = torch.zeros((B, V), dtype=torch.float32)
        logits[torch.arange(B), plan[:, t]] = 1.0
        nnops.gen_select_filtered(st, filt, logits.cuda(), V, ids, fin, lens, None, kept, cut, lp)
        nnops.gen_advance(st)
        R.select_ref(plan[:, t], h_ids, h_fin, h_len, t, P, eos, pad)
    torch.cuda.synchronize()
    assert torch.equal(ids.cpu(), h_ids) and torch.equal(fin.cpu(), h_fin) and torch.equal(lens.cpu(), h_len)
    assert torch.equal(ids[:, :P].cpu(), prompt)
    assert bool((kept[:, :Lmax - 1] == 1).all()) and torch.equal(cut[:, :Lmax - 1].cpu().long(), plan) and bool((lp[:, :Lmax - 1] == 0).all())
    assert bool((kept[:, Lmax - 1] == -3).all())
    # one step too many: t + 1 == Lmax stores no token
    nnops.gen_select_filtered(st, filt, torch.zeros((B, V), device="cuda"), V, ids, fin, lens, None, None, None, None)
    torch.cuda.synchronize()
    assert torch.equal(ids.cpu(), h_ids) and all(guards_intact(w) for w in frames)
    nnops.gen_advance(st)                                                    # t == Lmax: nothing at all
    nnops.gen_select_filtered(st, filt, torch.zeros((B, V), device="cuda"), V, ids, fin, lens, None, kept, cut, lp)
    torch.cuda.synchronize()
    assert torch.equal(ids.cpu(), h_ids) and all(guards_intact(w) for w in frames)


# ---------------------------------------------------------------------------------------------------------------- 11 refusals
def test_launcher_refuses_what_it_cannot_run():
    from kvq import _ffi, nnops
    from kvq._ffi import KvqError
    lib = _ffi.lib()
    B, V, ld = 2, 40, 40
    logits = torch.zeros((B, ld), device="cuda")
    ids = torch.zeros((B, LMAX), dtype=torch.int64, device="cuda")
    fin, lens = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    st, filt = state(0), nnops.new_gen_filter("cuda", 3, 0.5)
    good = [st.data_ptr(), filt.data_ptr(), logits.data_ptr(), ld, V, B, 0, ids.data_ptr(), fin.data_ptr(), lens.data_ptr(), None, None, None, None, None]
    assert lib.kvq_gen_select_filtered(*good) == 0
    for i in (0, 1, 2, 7, 8, 9):
        bad = list(good)
        bad[i] = None
        assert lib.kvq_gen_select_filtered(*bad) == -1 and b"null pointer" in lib.kvq_last_error()
    for i, v, text in ((3, 36, b"ld"), (3, 44, b"ld %"), (4, 0, b"positive"), (5, 0, b"positive"), (6, 7, b"io dtype"), (2, logits.data_ptr() + 4, b"aligned"),
                       (1, filt.data_ptr() + 2, b"misaligned"), (4, 32769, b"above"), (11, ids.data_ptr() + 2, b"misaligned")):
        bad = list(good)
        bad[i] = v
        if text == b"above":
            bad[3] = 32776
        assert lib.kvq_gen_select_filtered(*bad) == -1 and text in lib.kvq_last_error(), (i, lib.kvq_last_error())
    torch.cuda.synchronize()
    big = torch.zeros((1, 32776), device="cuda")
    with pytest.raises(KvqError, match="32768"):
        nnops.gen_select_filtered(st, filt, big, 32769, ids[:1], fin[:1], lens[:1])
    with pytest.raises(KvqError, match="filter state"):
        nnops.gen_select_filtered(st, torch.zeros(8, dtype=torch.int32, device="cuda"), logits, V, ids, fin, lens)
    with pytest.raises(KvqError, match="step_kept"):
        nnops.gen_select_filtered(st, filt, logits, V, ids, fin, lens, step_kept=torch.zeros((B, LMAX), device="cuda"))
    nnops.gen_select_filtered(st, filt, torch.zeros((1, 32768), device="cuda"), 32768, ids[:1], fin[:1], lens[:1])      # the capacity itself runs
    torch.cuda.synchronize()
