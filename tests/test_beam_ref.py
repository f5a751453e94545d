"""The beam-search reference of tests/_beam_ref.py, on the CPU: against an exhaustive search over every sentence of a toy model, its
tie rule, its bookkeeping (finished beams compete, dead beams, ancestry = parents), and the condition the GPU tests rest on -- the
seeds of their random cases leave at most 5 % of the (sentence, step) pairs undecided, judged by the numpy reference alone.
"""
import itertools

import numpy as np
import torch

import _beam_ref as BR


def toy_logits(prefix, V, seed):
    """the logits of a toy model that depends on the whole history"""
    return np.random.default_rng([seed] + [int(p) for p in prefix]).standard_normal(V) * 2.0


def search(V, W, L, seed, eos=None, pad=0):
    """the reference run on the toy model: one sentence, prompt [1]"""
    st = BR.new_state(1, W, L, [[1]], pad, R=W)
    for t in range(L - 1):
        x = np.stack([toy_logits(BR.gather_ref(st, t, pad)[r, :t + 1], V, seed) for r in range(W)])
        st, _, _ = BR.step_ref(st, x, V, W, t, 1, eos, pad)
    return st


def test_a_beam_as_wide_as_the_tree_finds_the_most_probable_sentences():
    V, L, seed = 2, 4, 5                                              # 2^3 = 8 sentences, W = 8 keeps them all
    st = search(V, 8, L, seed)
    hyp = BR.gather_ref(st, L - 1, 0)
    logp = {}
    for tail in itertools.product(range(V), repeat=L - 1):
        seq, s = [1], 0.0
        for v in tail:
            x = toy_logits(seq, V, seed)
            s += x[v] - BR.lse64(x)
            seq.append(v)
        logp[tuple(seq)] = s
    ranked = sorted(logp, key=lambda k: -logp[k])
    assert [tuple(h) for h in hyp.tolist()] == ranked
    np.testing.assert_allclose(st["scores"], [logp[k] for k in ranked], rtol=0, atol=1e-5)
    # a narrower beam: sorted scores, histories consistent with the parents
    st = search(7, 3, 6, 2)
    assert np.all(np.diff(st["scores"]) <= 0)
    hyp = BR.gather_ref(st, 5, 0)
    for r in range(3):
        assert np.array_equal(hyp[r], BR.backtrack(st["ids"], st["parent"], r, 5))
    greedy = search(7, 1, 6, 2)                                       # one beam: the arg-max at every step
    tokens = BR.gather_ref(greedy, 5, 0)[0]
    for t in range(5):
        assert tokens[t + 1] == int(np.argmax(toy_logits(tokens[:t + 1], 7, 2)))


def test_ties_dead_and_finished_beams():
    W, V, t = 3, 6, 1
    st = BR.new_state(1, W, 4, [[1]], 0, R=W)
    st["scores"][:] = [-1.0, -1.0, -np.inf]
    x = np.zeros((W, V))
    new, cands, decided = BR.step_ref(st, x, V, W, t, 1, 4, 0)
    assert [(c["w"], c["v"]) for c in cands[0][:3]] == [(0, 0), (0, 1), (0, 2)] and not decided[0]      # lower beam, then lower token
    st["finished"][0], st["lengths"][0] = 1, 2
    new, cands, _ = BR.step_ref(st, x, V, W, t, 1, 4, 0)
    assert cands[0][0]["fin"] and new["ids"][0, t + 1] == 0 and new["scores"][0] == -1.0 and new["lengths"][0] == 2
    assert new["parent"][:, t + 1].tolist() == [0, 1, 1] and new["finished"].tolist() == [1, 0, 0]
    x[1, 4] = 5.0                                                     # the end token wins in beam 1
    new, _, _ = BR.step_ref(st, x, V, W, t, 1, 4, 0)
    assert new["ids"][1, t + 1] == 4 and new["finished"][1] == 1 and new["lengths"][1] == t + 2
    x[1, 0] = np.nan                                                  # a NaN: the beam offers nothing, two dead beams follow
    new, _, _ = BR.step_ref(st, x, V, W, t, 1, 4, 0)
    assert new["scores"].tolist() == [-1.0, -np.inf, -np.inf] and new["finished"].tolist() == [1, 1, 1]
    same = BR.book(st, None, W, 3, 1, 4, 0)                           # t + 1 == L: nothing changes
    assert all(np.array_equal(same[k], st[k], equal_nan=True) for k in st)


def test_the_seeds_of_the_gpu_cases_leave_at_most_five_percent_undecided():
    pairs = undecided = 0
    for (V, ld, B, W, dtype) in BR.select_cases():
        st, x, t = BR.select_case(V, ld, B, W, dtype, BR.select_seed(V, W, dtype))
        seen = x.float().numpy()
        assert bool((x[:, V:].float() > 1e38).all())
        for b in range(B):
            pairs += 1
            undecided += not BR.is_decided(BR.candidates(st, seen, V, W, b), W)
    print(f"\n[beam reference] random select cases: {undecided} of {pairs} (sentence, step) pairs undecided")
    assert undecided <= 0.05 * pairs
    # the chained-steps case: the reference's own chain
    V, W, B, L, P = 2048, 4, 3, 8, 2
    for dtype in (torch.float32, torch.bfloat16):
        st = BR.new_state(B, W, L, np.random.default_rng(3).integers(0, V, (B, P)), 0)
        margin = np.inf
        for t, x in enumerate(BR.chain_logits(st["ids"].shape[0], V, 4, dtype)):
            st, cands, decided = BR.step_ref(st, x.float().numpy(), V, W, t, P, None, 0)
            assert all(decided[:B]), (dtype, t)
            for cs in cands[:B]:
                margin = min([margin] + [(a["s"] - b["s"]) / (2 * max(a["tol"], b["tol"])) for a, b in zip(cs, cs[1:])])
        print(f"[beam reference] chained steps {dtype}: smallest gap / (2 tol) = {margin:.1f}")
        assert margin > 2.0                                           # (so the kernel's f32 scores leave the steps decided as well)
