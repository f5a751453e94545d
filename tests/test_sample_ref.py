"""tests/_sample_ref.py -- the f64 reference of top-k / top-p filtered sampling -- against the installed transformers' own warpers
(TopKLogitsWarper then TopPLogitsWarper, as generate() chains them) on tie-free rows, and on the cases the warpers leave open:
ties, NaN, -inf, top_k >= V, a first token that already holds more than p.  No GPU."""
import pytest
import torch

import _sample_ref as S


def hf_kept(y, top_k, top_p):
    from transformers.generation.logits_process import TopKLogitsWarper, TopPLogitsWarper
    scores = y.clone()
    if top_k > 0:
        scores = TopKLogitsWarper(top_k=top_k)(None, scores)
    if top_p < 1.0:
        scores = TopPLogitsWarper(top_p=top_p)(None, scores)
    return scores > float("-inf")


@pytest.mark.parametrize("top_k", [0, 5, 50])
@pytest.mark.parametrize("top_p", [0.9, 0.5, 0.3, 1.0])
def test_reference_keeps_what_the_huggingface_warpers_keep(top_k, top_p):
    g = torch.Generator().manual_seed(1000 * top_k + int(100 * top_p))
    y = torch.randn((8, 200), generator=g) * 2.0
    assert all(len(set(r.tolist())) == 200 for r in y)                        # tie-free: the warpers' answer is determined
    ref = S.Cut(y, top_k, top_p)
    assert torch.equal(ref.kept(), hf_kept(y, top_k, top_p))
    assert torch.equal(ref.kept().sum(1), ref.n_keep)
    lo, hi = ref.keep_band()
    assert bool((lo <= ref.n_keep).all()) and bool((ref.n_keep <= hi).all())
    # the cut is the last kept column of the order, the probabilities sum to one over the set
    assert torch.equal(ref.rank.gather(1, ref.cut.unsqueeze(1)).squeeze(1) + 1, ref.n_keep)
    p = ref.probs()
    assert bool(((p > 0) == ref.kept()).all()) and torch.allclose(p.sum(1), torch.ones(8, dtype=torch.float64))
    lp, _ = ref.logprob(ref.order[:, 0])
    assert torch.allclose(lp, torch.log(p.gather(1, ref.order[:, :1]).squeeze(1)), atol=1e-12)


def test_ties_go_to_the_lower_index_and_the_cut_may_fall_inside_a_tied_group():
    y = torch.tensor([[1.0, 3.0, 1.0, 3.0, 1.0, 3.0, 0.0, 1.0]])
    order, n_valid = S.order_of(y)
    assert order.tolist() == [[1, 3, 5, 0, 2, 4, 7, 6]] and n_valid.tolist() == [8]
    for k, want in ((1, [1]), (2, [1, 3]), (4, [0, 1, 3, 5]), (5, [0, 1, 2, 3, 5])):
        ref = S.Cut(y, k, 1.0)
        assert ref.kept()[0].nonzero().view(-1).tolist() == want and int(ref.cut[0]) == order[0, k - 1] and int(ref.n_keep[0]) == k
    # every logit equal: the kept set is ids 0 .. k - 1; top-p keeps ceil(p V) of them
    flat = torch.full((1, 10), 0.25)
    assert S.Cut(flat, 3, 1.0).kept()[0].nonzero().view(-1).tolist() == [0, 1, 2]
    assert int(S.Cut(flat, 0, 0.35).n_keep[0]) == 4 and int(S.Cut(flat, 0, 0.35).cut[0]) == 3
    # -0 and +0 are one value
    z = torch.tensor([[0.0, -0.0, 0.0]])
    assert S.order_of(z)[0].tolist() == [[0, 1, 2]]


def test_nan_is_never_kept_or_counted_and_minus_inf_has_no_mass():
    nan, ninf = float("nan"), float("-inf")
    y = torch.tensor([[nan, 2.0, ninf, 1.0, nan, 0.0]])
    ref = S.Cut(y, 0, 1.0)
    assert ref.n_valid.tolist() == [4] and ref.order[0, :4].tolist() == [1, 3, 5, 2] and int(ref.n_keep[0]) == 4 and int(ref.cut[0]) == 2
    assert float(ref.probs()[0, 2]) == 0.0 and not bool(ref.kept()[0, [0, 4]].any())
    assert int(S.Cut(y, 10, 1.0).n_keep[0]) == 4                               # top_k >= n_valid: every valid column
    assert int(S.Cut(y, 3, 1.0).cut[0]) == 5
    ref = S.Cut(y, 0, 0.999999)
    assert int(ref.n_keep[0]) == 3                                             # the mass is complete before the -inf column
    empty = S.Cut(torch.full((1, 4), nan), 2, 0.5)
    assert empty.n_valid.tolist() == [0] and empty.n_keep.tolist() == [0] and empty.cut.tolist() == [-1]
    # a greedy state ignores the filters
    assert int(S.Cut(y, 1, 0.1, greedy=True).n_keep[0]) == 4


def test_top_k_at_and_above_v_and_a_first_token_that_already_holds_p():
    g = torch.Generator().manual_seed(5)
    y = torch.randn((3, 37), generator=g)
    for k in (37, 42):
        assert S.Cut(y, k, 1.0).n_keep.tolist() == [37] * 3
    assert S.Cut(y, 36, 1.0).n_keep.tolist() == [36] * 3
    peak = torch.zeros((1, 37))
    peak[0, 11] = 20.0
    ref = S.Cut(peak, 0, 0.9)
    assert ref.n_keep.tolist() == [1] and ref.cut.tolist() == [11]             # the token that crosses p is kept, and nothing else
    assert S.Cut(peak, 0, 2.0 ** -20).n_keep.tolist() == [1]
    # top-p inside top-k, renormalised: alone p = 0.5 of 4 equal tokens keeps 2, after top_k = 2 it keeps 1
    four = torch.zeros((1, 4))
    assert S.Cut(four, 0, 0.5).n_keep.tolist() == [2] and S.Cut(four, 2, 0.5).n_keep.tolist() == [1]
    # top_p outside (0, 1), a NaN included, is off
    for p in (1.0, 0.0, -0.5, 1.5, float("nan")):
        assert S.Cut(four, 3, p).n_keep.tolist() == [3]
    assert S.f32(0.9) != 0.9 and S.y_of(torch.tensor([[3.0]]), 0.0).tolist() == [[3.0]]
    assert S.chain_roundings()[:2] == (16, 50)
