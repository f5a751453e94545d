"""The reference of the free-running reconstruction metrics (tests/_seqcmp_ref.py) checked on its own -- known answers, an
exhaustive brute-force search, the metric's properties -- and the host arithmetic of kvq.census.ReconstructionCensus (slots_of,
result) on a hand-made table kept on the CPU.  No GPU."""
import itertools
import math
import random

import numpy as np
import pytest
import torch

import _seqcmp_ref as SR


def test_known_answers():
    d = lambda a, b: SR.edit_distance([ord(c) for c in a], [ord(c) for c in b])
    assert d("kitten", "sitting") == 3
    assert d("flaw", "lawn") == 2
    assert d("xabc", "abc") == 1 and d("abc", "xabc") == 1            # an insertion at the front: every position is shifted
    assert SR.positional_hits([9, 1, 2, 3], [1, 2, 3]) == 0
    assert d("", "") == 0 and d("", "abc") == 3 and d("abcd", "") == 4
    assert d("abc", "abc") == 0 and SR.positional_hits([1, 2, 3], [1, 2, 3]) == 3
    assert d("abc", "abd") == 1 and d("abc", "xyz") == 3


def test_against_an_exhaustive_search_on_two_symbols():
    seqs = [s for n in range(5) for s in itertools.product((0, 1), repeat=n)]
    assert len(seqs) == 31
    for h in seqs:
        for r in seqs:
            assert SR.edit_distance(h, r) == SR.brute_force_distance(h, r), (h, r)


def test_properties_bounds_symmetry_identity():
    rng = random.Random(0)
    for _ in range(300):
        A = rng.choice((2, 3, 50))
        h = [rng.randrange(A) for _ in range(rng.randrange(0, 20))]
        r = [rng.randrange(A) for _ in range(rng.randrange(0, 20))]
        d = SR.edit_distance(h, r)
        assert abs(len(h) - len(r)) <= d <= max(len(h), len(r))
        assert d == SR.edit_distance(r, h)
        assert (d == 0) == (h == r)
        assert SR.edit_distance(h, h) == 0


def test_seq_compare_record_skip_and_bad_rows():
    hyp = np.array([[7, 1, 2, 3, 99], [7, 1, 2, 99, 99], [7, 5, 5, 5, 5]])
    ref = np.array([[1, 2, 3, 99], [1, 2, 3, 4], [5, 5, 5, 5]])
    out, bad = SR.seq_compare(hyp, [4, 3, 0], ref, [3, 4, 4], hyp_skip=1, Lmax=4)
    assert out.tolist() == [[0, 3, 3, 3], [2, 2, 2, 4], [-1, 0, 0, 0]] and bad == 1
    out, bad = SR.seq_compare(hyp, [5, 5, 5], ref, [4, 5, 4], hyp_skip=1, Lmax=4)
    assert out[1].tolist() == [-1, 0, 0, 0] and bad == 1 and out[2].tolist() == [0, 4, 4, 4]


def test_accumulate_is_a_scatter_add():
    per = np.array([[0, 3, 3, 3], [2, 1, 2, 4], [-1, 0, 0, 0], [1, 0, 5, 4]], dtype=np.int32)
    slot = np.array([[0, 1], [0, 2], [0, 1], [0, 3]], dtype=np.int32)
    t = SR.accumulate(per, slot, np.zeros((3, 6), dtype=np.int64))
    assert t.tolist() == [[3, 1, 3, 4, 10, 11], [1, 1, 0, 3, 3, 3], [1, 0, 2, 1, 2, 4]]      # slot 3 = R is skipped, row 2 (dist -1) too


def test_census_slots_of_lays_factors_out_by_prefix_sums():
    from kvq.census import ReconstructionCensus
    c = ReconstructionCensus([2, 3], device="cpu")
    assert c.R == 6 and c.offsets == [1, 3]
    assert c.rows() == [(None, None), (0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]
    labels = torch.tensor([[0, 0], [1, 2], [2, 1], [0, -1], [-1, 3]])
    s = c.slots_of(labels)
    assert s.dtype == torch.int32 and s.tolist() == [[0, 1, 3], [0, 2, 5], [0, -1, 4], [0, 1, -1], [0, -1, -1]]
    none = ReconstructionCensus(device="cpu")
    assert none.R == 1 and none.slots_of(torch.zeros((4, 0), dtype=torch.int64)).tolist() == [[0]] * 4
    from kvq._ffi import KvqError
    with pytest.raises(KvqError, match="labels"):
        c.slots_of(torch.zeros((4, 3), dtype=torch.int64))
    with pytest.raises(KvqError, match="cardinalities"):
        ReconstructionCensus([2, 0], device="cpu")
    with pytest.raises(KvqError, match="limits"):
        ReconstructionCensus([4096], device="cpu")


def test_census_result_arithmetic_on_a_hand_made_table():
    from kvq.census import ReconstructionCensus
    c = ReconstructionCensus([2], device="cpu")
    #                         sentences exact dist hits hyp ref
    c.table.copy_(torch.tensor([[4, 1, 6, 30, 44, 40], [4, 1, 6, 30, 44, 40], [0, 0, 0, 0, 0, 0]]))
    c.n_bad.fill_(2)
    r = c.result()
    assert r["sentences"].tolist() == [4, 4, 0] and r["n_bad"] == 2 and r["rows"] == [(None, None), (0, 0), (0, 1)]
    for k, want in (("exact", 0.25), ("token_acc", 0.75), ("edit_rate", 0.15), ("len_ratio", 1.1)):
        assert r[k].dtype == torch.float64 and r[k][0].item() == want and r[k][1].item() == want, k
        assert math.isnan(r[k][2].item()), k
    c.reset()
    assert not bool(c.table.any()) and int(c.n_bad) == 0 and math.isnan(c.result()["exact"][0].item())
