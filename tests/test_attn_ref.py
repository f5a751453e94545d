"""The attention checker checked (tests/_attn_ref.py), without a GPU: the rounding model equals the f64 reference once its
roundings are switched off, and the per-row judge -- with the model standing in for the kernel -- accepts the model's own output
at margin 1 and rejects every planted bug at the margins committed for the GPU tests."""
import pytest
import torch

import _attn_ref as A
from _dropout_ref import attend_allowed, masked_softmax

B, NH = 4, 3


def _case(S, causal, p, family, Sk=None, seed=0):
    Sk = S if Sk is None else Sk
    g = torch.Generator().manual_seed(1000 * S + 10 * Sk + seed)
    bf = lambda *shape: torch.randn(*shape, generator=g).bfloat16()
    lens = torch.tensor([Sk, 1, max(2, Sk // 2 - 1), max(1, Sk - 3)])          # lengths include 1 and S
    mask = (torch.arange(Sk)[None] < lens[:, None]).long()
    keep = (torch.rand(B, NH, S, Sk, generator=g) >= p).double() if p > 0 else None
    return dict(q=bf(B, NH, S, 64), k=bf(B, NH, Sk, 64), v=bf(B, NH, Sk, 64), g_out=bf(B, NH, S, 64), mask=mask, causal=causal,
                scale=0.125, keep=keep, p=p, family=family)


def _args(c):
    return c["q"], c["k"], c["v"], c["mask"], c["causal"], c["scale"], c["keep"], c["p"], c["g_out"]


CASES = [(S, causal, p, family) for family in ("mfma", "blk") for S in (12, 32) for causal in (False, True) for p in (0.0, 0.1)]
CASES += [(40, causal, 0.1, "blk") for causal in (False, True)]               # two key blocks: the running-softmax roundings


@pytest.mark.parametrize("S,causal,p,family", CASES)
def test_model_without_roundings_is_the_reference(S, causal, p, family):
    c = _case(S, causal, p, family)
    ref = A.reference(*_args(c))
    mod = A.model(*_args(c), family=family, rounding=False)
    for name in A.OUTPUTS + ("lse",):
        want = ref["g_" + name[-1]].sum(2) if name.startswith("pb_") else ref[name]      # (the reference's partials sum rounded rows)
        scale = max(1.0, float(want.abs().max()))
        assert float((mod[name] - want).abs().max()) <= 1e-11 * scale, name
    for name in "qkv":                                   # reference partials are sums of the bf16-rounded rows
        torch.testing.assert_close(ref["pb_" + name], A.rbf(ref["g_" + name]).sum(2), rtol=0, atol=0)


@pytest.mark.parametrize("S,causal,p,family", CASES)
def test_judge_accepts_the_model_and_rejects_every_mutation(S, causal, p, family):
    c = _case(S, causal, p, family)
    ref = A.reference(*_args(c))
    mod = A.model(*_args(c), family=family)
    ratios = A.judge_all(mod, ref, mod, {"fwd": 1.0, "bwd": 1.0}, "model")
    assert max(ratios.values()) <= 1.0
    for name, mutate in A.MUTATIONS.items():
        bad = mutate(c)
        if bad is None:                                   # this case cannot show the bug (no dropout / not causal / no padding)
            continue
        with pytest.raises(AssertionError):
            A.judge_all(bad, ref, mod, A.MARGIN[family], name)
        t = A.MUTATION_TARGET[name]                       # ... and by the row envelope of the output it hits, not by the lse check
        with pytest.raises(AssertionError, match="worst"):
            A.judge(bad[t], ref[t], mod[t], t, A.MARGIN[family][A.FAMILY_OF[t]])


def test_every_mutation_is_exercised():
    """No mutation is skipped by every case."""
    seen = set()
    for S, causal, p, family in CASES:
        c = _case(S, causal, p, family)
        seen |= {n for n, m in A.MUTATIONS.items() if m(c) is not None}
    assert seen == set(A.MUTATIONS)


def test_cross_attention_shapes_and_empty_rows():
    """Sq != Sk, and a sentence without any attended key: zero probabilities, zero gradients, lse = log(1e-37), no NaN anywhere."""
    c = _case(9, False, 0.1, "mfma", Sk=12)
    c["mask"][3] = 0
    ref = A.reference(*_args(c))
    for fam in ("mfma", "blk"):
        mod = A.model(*_args(c), family=fam)
        for name in A.OUTPUTS + ("lse",):
            assert torch.isfinite(ref[name]).all() and torch.isfinite(mod[name]).all(), name
        for name in ("ctx", "g_q", "g_k", "g_v", "pb_q", "pb_k", "pb_v"):
            assert not ref[name][3].any() and not mod[name][3].any(), name
        assert torch.all(ref["lse"][3] == A.LSE_EMPTY) and torch.all(mod["lse"][3] == A.LSE_EMPTY)
        A.judge_all(mod, ref, mod, {"fwd": 1.0, "bwd": 1.0}, fam)


def test_one_convention_with_ref_step():
    """reference() and _dropout_ref.ref_step() share attend_allowed / masked_softmax / dropout_scale; the empty-row extension
    changes nothing where a row attends to something."""
    torch.manual_seed(3)
    s = torch.randn(2, 3, 7, 9, dtype=torch.float64)
    mask = torch.tensor([[1, 1, 1, 0, 1, 0, 0, 0, 0], [1] * 9])
    allow = attend_allowed(2, 7, 9, mask, False, s.device).expand(2, 3, 7, 9)
    assert torch.equal(masked_softmax(s, allow), masked_softmax(s, allow, empty_rows_zero=True))
    assert torch.equal(masked_softmax(s, allow), torch.softmax(s.masked_fill(~allow, float("-inf")), -1))


def test_judge_reports_the_worst_row():
    ref = torch.randn(2, 3, 5, 64, dtype=torch.float64)
    mod = A.rbf(ref)
    got = mod.clone()
    got[1, 2, 4, 7] += 1.0
    with pytest.raises(AssertionError, match=r"'sentence': 1, 'head': 2, 'row': 4, 'column': 7"):
        A.judge(got, ref, mod, "x", 4.0)
    got = mod.clone()
    got[0, 0, 0, 0] = float("nan")
    with pytest.raises(AssertionError):
        A.judge(got, ref, mod, "x", 1e9)


def test_zero_reference_rows_get_the_cancellation_floor_and_nothing_else_does():
    """A sentence of one token without dropout: g_q and g_k are exactly zero (P = 1, dS = 0).  f32 summation noise below the floor
    passes there; the same noise on top of a non-zero row is judged by the envelope alone, and noise above the floor fails."""
    c = _case(32, False, 0.0, "blk")
    ref = A.reference(*_args(c))
    mod = A.model(*_args(c), family="blk")
    assert not ref["g_q"][1].any() and not mod["g_q"][1].any()          # sentence 1 has length 1
    floors = A.cancellation_floors(c["q"], c["k"], c["v"], c["g_out"], c["mask"], False, 0.125)
    assert 0 < float(floors["g_q"][1].max()) < 5e-4 and 0 < float(floors["pb_q"][1].max()) < 32 * 5e-4
    assert not floors["g_q"][0].any() and not floors["g_k"][0].any()      # a full sentence has no single-key query: no floor at all
    big = {S: A.cancellation_floors(*(_case(S, True, 0.0, "blk")[n] for n in ("q", "k", "v", "g_out", "mask")), True, 0.125) for S in (32, 128)}
    assert all(float(f["g_q"].max()) < 5e-4 and float(f["g_k"].max()) < 32 * 5e-4 for f in big.values())   # does not grow with S
    got = {n: t.clone() for n, t in mod.items()}
    got["g_q"][1] += 0.5 * floors["g_q"][1]
    with pytest.raises(AssertionError):
        A.judge_all(got, ref, mod, A.MARGIN["blk"], "no floor")
    A.judge_all(got, ref, mod, {"fwd": 1.0, "bwd": 1.0}, "floor", floors=floors)
    got["g_q"][1] += 20 * floors["g_q"][1]
    with pytest.raises(AssertionError):
        A.judge_all(got, ref, mod, A.MARGIN["blk"], "above", floors=floors)
