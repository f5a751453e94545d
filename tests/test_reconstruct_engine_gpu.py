"""TrainEngine.reconstruct and kvq.census.ReconstructionCensus on the engine: encode -> generate -> kvq_seq_compare
[-> kvq_seq_compare_accumulate], against the same calls made by hand and the plain Python DP of tests/_seqcmp_ref.py.

Models: kvq-bert-tiny, built as tests/test_latent_engine_gpu.py builds them (Shelgon with a VectorQuantizer, Bagon), bf16 and f32,
B = 6, S = 12.  Everything compared here is an integer: equality, no tolerance.  An untrained model reproduces nothing, so the
exact-match path is driven with targets made from what the model generates; the end token of the eos cases is a token the model
does generate (taken from its own output), so that sentences end before max_length.
"""
import functools

import numpy as np
import pytest
import torch

import _seqcmp_ref as SR
from test_latent_engine_gpu import B, S, batch, build

pytestmark = pytest.mark.gpu

START, V = 101, 2048
CASES = [("shelgon", torch.float32), ("shelgon", torch.bfloat16), ("bagon", torch.float32), ("bagon", torch.bfloat16)]
EOS = [False, True]


@functools.lru_cache(maxsize=None)
def case(kind, dtype):
    from kvq.engine import engine_of
    model = build(kind)
    model.compute_dtype = dtype
    model = model.cuda().eval()
    eng = engine_of(model)
    assert eng.dtype == dtype
    e, em = batch(kind, 1)[:2]
    fixed = batch(kind, 2)
    with torch.no_grad():
        before = eng.forward_logits(*fixed)["logits"].clone()
        free = by_hand(eng, e, em, None)
    eos = int(free["ids"][0, 6])                    # a token the model writes: sentence 0 ends at column 6 or earlier
    return dict(eng=eng, e=e, em=em, fixed=fixed, before=before, eos=eos)


def by_hand(eng, e, em, eos, beams=1, length_penalty=0.0):
    enc = eng.encode(e, em)
    lat = (enc["z_q"] if eng.has_vq else enc["z"]).reshape(e.shape[0], e.shape[1], eng.H)
    prompt = torch.full((e.shape[0], 1), START, dtype=torch.int64, device="cuda")
    if beams == 1:
        return eng.generate(lat, e.shape[1] + 1, prompt, eos_id=eos)
    return eng.beam_search(lat, e.shape[1] + 1, prompt, beams, eos_id=eos, length_penalty=length_penalty)


def reference(ids, lengths, tgt, ref_len):
    out, bad = SR.seq_compare(ids.cpu().numpy(), lengths.cpu().tolist(), tgt.cpu().numpy(), ref_len, hyp_skip=1, Lmax=max(ids.shape[1] - 1, tgt.shape[1]))
    assert bad == 0
    return out


def assert_metrics(rec, want):
    got = torch.stack([rec["dist"], rec["hits"], rec["hyp_len"], rec["ref_len"]], dim=1).cpu().numpy()
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    assert rec["exact"].dtype == torch.bool and rec["exact"].cpu().tolist() == [bool(d == 0) for d in want[:, 0]]
    assert rec["n_bad"].dtype == torch.int64 and int(rec["n_bad"]) == 0


def ref_lengths(c, eos, mask=None):
    return [S] * B if eos is None else (c["em"] if mask is None else mask).sum(1).cpu().tolist()


@pytest.mark.parametrize("with_eos", EOS)
@pytest.mark.parametrize("kind,dtype", CASES)
def test_reconstruct_is_encode_generate_compare_by_hand(kind, dtype, with_eos):
    c = case(kind, dtype)
    eng, e, em = c["eng"], c["e"], c["em"]
    eos = c["eos"] if with_eos else None
    with torch.no_grad():
        rec = eng.reconstruct(e, em, START, eos_id=eos, want_ids=True)
        gen = by_hand(eng, e, em, eos)
    assert rec["ids"].shape == (B, S + 1) and torch.equal(rec["ids"], gen["ids"]) and torch.equal(rec["lengths"], gen["lengths"])
    if with_eos:
        assert int(gen["lengths"][0]) <= 7 and bool(gen["finished"][0])
    else:
        assert gen["lengths"].tolist() == [S + 1] * B
    assert_metrics(rec, reference(gen["ids"], gen["lengths"], e, ref_lengths(c, eos)))
    assert set(eng.reconstruct(e, em, START, eos_id=eos)) == {"dist", "hits", "hyp_len", "ref_len", "exact", "n_bad"}


@pytest.mark.parametrize("with_eos", EOS)
@pytest.mark.parametrize("kind,dtype", CASES)
def test_targets_made_from_the_models_own_sentence(kind, dtype, with_eos):
    c = case(kind, dtype)
    eng, e, em = c["eng"], c["e"], c["em"]
    eos = c["eos"] if with_eos else None
    with torch.no_grad():
        gen = by_hand(eng, e, em, eos)
        own = gen["ids"][:, 1:]                                           # a view with row stride S + 1: the stride is what is read
        n = gen["lengths"] - 1
        own_mask = (torch.arange(S, device="cuda")[None] < n[:, None]).long()
        rec = eng.reconstruct(e, em, START, eos_id=eos, target_ids=own, target_mask=own_mask)
    assert rec["dist"].tolist() == [0] * B and bool(rec["exact"].all())
    assert rec["hits"].tolist() == n.tolist() and rec["hyp_len"].tolist() == n.tolist() == rec["ref_len"].tolist()
    # one token deleted in sentence 0, one substituted in sentence 1
    tgt, mask = own.clone(), own_mask.clone()
    tgt[0, :-1] = own[0, 1:]
    tgt[0, -1] = 0
    mask[0, int(n[0]) - 1] = 0
    tgt[1, 0] = (own[1, 0] + 1) % V
    with torch.no_grad():
        rec = eng.reconstruct(e, em, START, eos_id=eos, target_ids=tgt, target_mask=mask)
    want = reference(gen["ids"], gen["lengths"], tgt, ref_lengths(c, eos, mask))
    assert_metrics(rec, want)
    if with_eos:
        assert rec["dist"].tolist() == [1, 1] + [0] * (B - 2) and rec["exact"].tolist() == [False, False] + [True] * (B - 2)
        assert int(rec["ref_len"][0]) == int(n[0]) - 1 and int(rec["hits"][1]) == int(n[1]) - 1
    else:
        assert int(rec["dist"][1]) == 1 and rec["dist"][2:].tolist() == [0] * (B - 2)


@pytest.mark.parametrize("kind,dtype", [("shelgon", torch.bfloat16), ("bagon", torch.float32)])
def test_three_beams_score_the_best_hypothesis_of_beam_search(kind, dtype):
    c = case(kind, dtype)
    eng, e, em, eos = c["eng"], c["e"], c["em"], c["eos"]
    with torch.no_grad():
        rec = eng.reconstruct(e, em, START, eos_id=eos, num_beams=3, length_penalty=1.0, want_ids=True)
        beams = by_hand(eng, e, em, eos, beams=3, length_penalty=1.0)
    assert torch.equal(rec["ids"], beams["ids"]) and torch.equal(rec["lengths"], beams["lengths"])
    assert_metrics(rec, reference(beams["ids"], beams["lengths"], e, ref_lengths(c, eos)))


@pytest.mark.parametrize("kind,dtype", [("shelgon", torch.bfloat16), ("bagon", torch.float32)])
def test_census_over_two_batches_is_the_sum_of_the_sentences(kind, dtype):
    from kvq.census import ReconstructionCensus
    c = case(kind, dtype)
    eng, eos = c["eng"], c["eos"]
    census = ReconstructionCensus([2, 3])
    want = np.zeros((6, 6), dtype=np.int64)
    g = torch.Generator().manual_seed(5)
    for seed in (1, 3):
        e, em = batch(kind, seed)[:2]
        labels = torch.stack([torch.randint(0, 2, (B,), generator=g), torch.randint(0, 3, (B,), generator=g)], dim=1)
        labels[2, 1] = 3                                                 # outside its factor's range: counted in row 0 and factor 0 only
        slots = census.slots_of(labels)
        assert slots.device.type == "cuda" and slots[2].tolist() == [0, 1 + int(labels[2, 0]), -1]
        with torch.no_grad():
            rec = eng.reconstruct(e, em, START, eos_id=eos, slots=slots, census=census)
        per = torch.stack([rec["dist"], rec["hits"], rec["hyp_len"], rec["ref_len"]], dim=1).cpu().numpy()
        SR.accumulate(per, slots.cpu().numpy(), want)
    assert np.array_equal(census.table.cpu().numpy(), want)
    assert want[0, 0] == 2 * B and want[1:3, 0].sum() == 2 * B and want[3:, 0].sum() == 2 * B - 2
    res = census.result()
    assert res["n_bad"] == 0 and res["sentences"].tolist() == want[:, 0].tolist()
    assert res["token_acc"][0].item() == want[0, 3] / want[0, 5] and res["edit_rate"][0].item() == want[0, 2] / want[0, 5]
    # without slots every sentence goes to row 0
    census.reset()
    with torch.no_grad():
        rec = eng.reconstruct(c["e"], c["em"], START, census=census)
    assert census.table[0].tolist() == [B, int(rec["exact"].sum()), int(rec["dist"].sum()), int(rec["hits"].sum()), B * S, B * S]
    assert not bool(census.table[1:].any())


@pytest.mark.parametrize("kind,dtype", CASES)
def test_the_engines_state_does_not_move(kind, dtype):
    c = case(kind, dtype)
    eng = c["eng"]
    with torch.no_grad():
        eng.reconstruct(c["e"], c["em"], START, eos_id=c["eos"])
        eng.reconstruct(c["e"], c["em"], START, num_beams=2)
        after = eng.forward_logits(*c["fixed"])["logits"]
    assert torch.equal(after, c["before"])


def test_refusals_name_the_argument(monkeypatch):
    from kvq._ffi import KvqError
    from kvq.census import ReconstructionCensus
    from kvq.engine import SamplingRefused
    c = case("shelgon", torch.float32)
    eng, e, em = c["eng"], c["e"], c["em"]
    census = ReconstructionCensus([2])
    slots = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    for kw, text in ((dict(start_id=-1), "start_id"), (dict(start_id=V), "start_id"), (dict(start_id=1.0), "start_id"), (dict(eos_id=V), "eos_id"),
                     (dict(target_mask=em), "target_mask"), (dict(target_ids=e[:3]), "target_ids"), (dict(target_ids=e.int()), "target_ids"),
                     (dict(target_ids=e, eos_id=102), "target_mask"), (dict(target_ids=e, target_mask=em[:, :5]), "target_mask"),
                     (dict(slots=slots), "slots"), (dict(census="x"), "census"), (dict(census=ReconstructionCensus([2], device="cpu")), "census"),
                     (dict(census=census, slots=slots.long()), "slots"), (dict(census=census, slots=slots[:3]), "slots"),
                     (dict(num_beams=0), "num_beams"), (dict(num_beams=2, length_penalty=float("nan")), "length_penalty"),
                     (dict(max_length=0), "max_length"), (dict(max_length=65), "max_length"), (dict(max_length=40), "sequence length")):
        args = dict(start_id=START)
        args.update(kw)
        with pytest.raises(KvqError, match=text):
            eng.reconstruct(e, em, **args)
    with pytest.raises(KvqError, match="enc_mask"):
        eng.reconstruct(e, em[:, :5], START)
    for kw in (dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9, seed=3), dict(want_scores=True)):
        with pytest.raises(SamplingRefused, match="|".join(kw)):
            eng.reconstruct(e, em, START, **kw)
    with pytest.raises(TypeError, match="bogus"):
        eng.reconstruct(e, em, START, bogus=1)
    assert not bool(census.table.any())
    monkeypatch.setattr(eng, "fp8", True)
    with pytest.raises(KvqError, match="reconstruct.*fp8"):
        eng.reconstruct(e, em, START)
    monkeypatch.setattr(eng, "fp8", False)
    monkeypatch.setattr(eng, "group", object())
    with pytest.raises(KvqError, match="reconstruct.*single-process"):
        eng.reconstruct(e, em, START)
