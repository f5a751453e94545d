"""TrainEngine.attention_maps / AttentionCensus against HuggingFace's output_attentions=True.

Models: kvq-bert-tiny (2 layers, 2 heads), B = 6, S = 12: Shelgon (VectorQuantizer, K = 32) on the autoencoding call and Bagon with
decoder ids != encoder ids, in f32 and bf16.  The query projections are scaled by 4 after the default initialisation (std 0.02 gives
scores of ~0.05, i.e. maps within a few per cent of uniform, where no two layers or heads differ by much).
Reference: the model's own HF modules with set_attn_implementation("eager"), wired as the reference's
analyses/cross_attention/extract_model_cross_attention.py:73-83, in f32; for the bf16 engine on the bf16-rounded weights; the
decoder is conditioned on the codebook rows of the ENGINE's indices, so a quantiser flip is not counted as an attention error.

Tolerance of the per-sentence maps: not derivable in advance (the engine's whole forward stands between the inputs and the maps),
so measured on an MI355X and doubled -- worst |engine - HF| over both families and both models:
    f32   measured 8.941e-08 (Shelgon and Bagon alike: 1.5 ulp of a probability in [0.5, 1))   bound 1.788e-07
    bf16  measured 1.304e-03 (Shelgon; Bagon 9.156e-04)                                         bound 2.608e-03
against 1.5e-01 (layers swapped), 1.7e-01 (heads swapped) and 9.2e-01 (cross and self exchanged) for the three wrong maps below.
Each bound must discriminate: HF's own maps with the two layers swapped, the two heads swapped, and cross / self exchanged
differ from HF's maps by at least 10 x the bound (asserted).
"""
import copy
import functools
import os
import subprocess
import sys

import pytest
import torch

from _gemm_guard import forbid_vendor_gemms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")

MEASURED = {torch.float32: 8.941e-08, torch.bfloat16: 1.304e-03}          # worst |engine - HF| seen on the card (see the header)
BOUND = {dt: 2 * m for dt, m in MEASURED.items()}
B, S = 6, 12


def _build(kind):
    from models.bagon.Bagon import Bagon
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(0)
    if kind == "bagon":
        model = Bagon("kvq-bert-tiny", "kvq-bert-tiny", True, compute_dtype=torch.float32)
    else:
        vq = VectorQuantizer(32, 128, 0.25, vq_codebook_init_values=torch.randn(32, 128))
        vq.materialize_min_encodings = False
        model = Shelgon("kvq-bert-tiny", vq, "kvq-bert-tiny", None, compute_dtype=torch.float32)
    with torch.no_grad():
        for l in list(model.encoder.encoder.layer) + list(model.decoder.bert.encoder.layer):
            l.attention.self.query.weight.mul_(4.0)
            if hasattr(l, "crossattention"):
                l.crossattention.self.query.weight.mul_(4.0)
    return model


def _batch(kind, seed):
    """(enc ids, enc mask, dec ids, dec mask); Shelgon: the decoder reads the encoder's ids (None, None)"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(3, S + 1, (B,), generator=g)
    keep = torch.arange(S)[None] < lens[:, None]
    e = (torch.randint(1000, 2000, (B, S), generator=g) * keep).cuda()
    em = keep.long().cuda()
    if kind != "bagon":
        return e, em, None, None
    noise = torch.randint(1000, 2000, (B, S), generator=g).cuda()
    flip = (torch.rand(B, S, generator=g) < 0.3).cuda()
    d = torch.where(flip, noise, e) * em
    assert not torch.equal(d, e)
    return e, em, d, em.clone()


def _hf_maps(ref, e, em, d, dm, indices):
    """{family: f32 [L, B, nh, S, S]} from HF's eager attention, wired as the reference's script (:73-83)"""
    with torch.no_grad():
        enc = ref.encoder(e, attention_mask=em, output_attentions=True)
        cond = enc.last_hidden_state
        if indices is not None:
            cond = ref.vector_quantizer.embedding.weight[indices.reshape(-1)].view(cond.shape)
        out = ref.decoder(encoder_hidden_states=cond, input_ids=e if d is None else d, attention_mask=em if dm is None else dm,
                          output_attentions=True)
    return {"cross": torch.stack(out.cross_attentions, 0), "dec_self": torch.stack(out.attentions, 0), "enc_self": torch.stack(enc.attentions, 0)}


@functools.lru_cache(maxsize=None)
def case(kind, dtype):
    """model + engine in `dtype`, three batches, the engine's per-sentence maps of each and HF's of the first"""
    from kvq.engine import engine_of
    model = _build(kind)
    ref = copy.deepcopy(model)                                     # f32 HF modules; for the bf16 engine on the weights it computes with
    if dtype == torch.bfloat16:
        with torch.no_grad():
            for p in ref.parameters():
                p.copy_(p.bfloat16().float())
    ref = ref.cuda().eval()
    for m in (ref.encoder, ref.decoder):
        m.set_attn_implementation("eager")
    model.compute_dtype = dtype
    model = model.cuda().eval()
    eng = engine_of(model)
    assert eng.dtype == dtype
    batches = [_batch(kind, seed) for seed in (1, 2, 3)]
    with torch.no_grad():
        logits_before = eng.forward_logits(*batches[0])
        maps = [model.attention_maps(*b, per_sentence=True) if kind == "bagon" else model.attention_maps(b[0], b[1], per_sentence=True)
                for b in batches]
        logits_after = eng.forward_logits(*batches[0])
    hf = _hf_maps(ref, *batches[0], logits_before["indices"])
    torch.cuda.synchronize()
    return dict(model=model, eng=eng, batches=batches, maps=maps, hf=hf, logits_before=logits_before["logits"], logits_after=logits_after["logits"])


KINDS = [("shelgon", torch.float32), ("shelgon", torch.bfloat16), ("bagon", torch.float32), ("bagon", torch.bfloat16)]


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_per_sentence_maps_equal_huggingface_output_attentions(kind, dtype):
    c = case(kind, dtype)
    got, hf = c["maps"][0], c["hf"]
    assert set(got) == {"dec_self", "cross"}
    worst = 0.0
    for f in got:
        assert got[f].shape == hf[f].shape == (2, B, 2, S, S) and got[f].dtype == torch.float32
        assert not bool(torch.isnan(got[f]).any())
        worst = max(worst, float((got[f] - hf[f]).abs().max()))
    # what a wrong map would look like, on HF's own output: layers swapped, heads swapped, cross and self exchanged
    wrong = {"layers swapped": max(float((hf[f].flip(0) - hf[f]).abs().max()) for f in got),
             "heads swapped": max(float((hf[f].flip(2) - hf[f]).abs().max()) for f in got),
             "cross and self exchanged": float((hf["cross"] - hf["dec_self"]).abs().max())}
    print(f"\n[attention_maps] {kind} {dtype}: worst |engine - HF| = {worst:.3e} (bound {BOUND[dtype]}); " +
          ", ".join(f"{k} {v:.3e}" for k, v in wrong.items()))
    assert worst <= BOUND[dtype]
    for what, diff in wrong.items():
        assert diff >= 10 * BOUND[dtype], f"{what}: {diff} does not stand out from the bound {BOUND[dtype]}"


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_census_over_three_batches_equals_the_mean_of_the_per_sentence_maps(kind, dtype):
    from kvq.census import AttentionCensus
    c = case(kind, dtype)
    eng = c["eng"]
    census = AttentionCensus(2, 2, S, S, families=("dec_self", "cross", "enc_self"))
    stacks = []
    with torch.no_grad():
        for b in c["batches"]:
            assert eng.attention_maps(*b, census=census) is None
        for b in c["batches"]:                                  # the same families once more, per sentence (enc_self included)
            stacks.append(eng.attention_maps(*b, census=AttentionCensus(2, 2, S, S, families=("dec_self", "cross", "enc_self")),
                                             per_sentence=True))
    assert census.count == 3 * B
    res = census.results()
    assert set(res) == {"dec_self", "cross", "enc_self"}
    for f, mean in res.items():
        want = torch.cat([s[f] for s in stacks], 1).double().mean(1)               # [L, 18, nh, S, S] -> mean over the 18 sentences
        assert mean.shape == (2, 2, S, S) and mean.dtype == torch.float32 and not mean.is_cuda
        assert float((mean.double() - want.cpu()).abs().max()) <= 1e-6, f
    for f in ("dec_self", "cross"):                             # and the per-sentence maps do not depend on what else was asked for
        for s, m in zip(stacks, c["maps"]):
            assert torch.equal(s[f], m[f])
    hf_enc = c["hf"]["enc_self"]
    assert float((stacks[0]["enc_self"] - hf_enc).abs().max()) <= BOUND[dtype]


@pytest.mark.parametrize("kind,dtype", KINDS)
def test_forward_logits_are_bit_identical_before_and_after(kind, dtype):
    c = case(kind, dtype)
    assert torch.equal(c["logits_before"], c["logits_after"])


@pytest.mark.parametrize("kind", ["shelgon", "bagon"])
def test_bf16_maps_run_without_vendor_gemms_and_repeat_bit_for_bit(kind, monkeypatch):
    c = case(kind, torch.bfloat16)
    b = c["batches"][0]
    with monkeypatch.context() as mp:
        forbid_vendor_gemms(mp)
        with torch.no_grad():
            again = c["eng"].attention_maps(*b, per_sentence=True)
        torch.cuda.synchronize()
    for f, t in again.items():
        assert torch.equal(t, c["maps"][0][f])


def test_step_graph_is_unchanged_by_an_attention_maps_call():
    from kvq.census import AttentionCensus
    from kvq.engine import TrainEngine
    model = _build("shelgon")
    model.compute_dtype = torch.bfloat16
    model = model.cuda().train()
    eng = TrainEngine(model, lr=1e-3)
    e, em, _, _ = _batch("shelgon", 4)
    for _ in range(5):
        eng.train_step(e, em)
    torch.cuda.synchronize()
    assert eng._graphs, "the step was not captured"
    keys = list(eng._graphs)
    before = [g.node_census() for g in eng._graphs.values()]
    census = AttentionCensus(2, 2, S, S)
    maps = eng.attention_maps(e, em, census=census, per_sentence=True)
    out = eng.train_step(e, em)
    torch.cuda.synchronize()
    assert list(eng._graphs) == keys and [g.node_census() for g in eng._graphs.values()] == before
    assert torch.isfinite(out["loss_recon"]) and census.count == B and maps["cross"].shape == (2, B, 2, S, S)
    assert model.training                                       # the call is an evaluation pass; it leaves the module's mode alone


def test_refusals():
    from kvq._ffi import KvqError
    from kvq.census import AttentionCensus
    c = case("shelgon", torch.float32)
    eng, (e, em, _, _) = c["eng"], c["batches"][0]
    with pytest.raises(KvqError, match="census"):
        eng.attention_maps(e, em)
    long_ids = torch.randint(1000, 2000, (2, 40), device="cuda")
    with pytest.raises(KvqError, match="sequence length"):      # f32 ends at 32 tokens: what forward_logits refuses too
        eng.attention_maps(long_ids, torch.ones_like(long_ids), per_sentence=True)
    with pytest.raises(KvqError, match="AttentionCensus"):      # a table of another shape: refused before anything is launched
        eng.attention_maps(e, em, census=AttentionCensus(2, 2, S + 1, S))
    wrong = AttentionCensus(3, 2, S, S)
    with pytest.raises(KvqError, match="AttentionCensus"):
        eng.attention_maps(e, em, census=wrong)
    assert wrong.count == 0 and float(wrong.tables["cross"].abs().max()) == 0.0
    eng._cap = object()                                         # as while a step is being captured
    try:
        with pytest.raises(KvqError, match="graph capture"):
            eng.attention_maps(e, em, per_sentence=True)
    finally:
        eng._cap = None
    eng.group = object()                                        # as with a process group
    try:
        with pytest.raises(KvqError, match="process group"):
            eng.attention_maps(e, em, per_sentence=True)
    finally:
        eng.group = None
    assert eng._maps is None
    with pytest.raises(KvqError, match="no sentence"):
        AttentionCensus(2, 2, S, S).results()


def test_analysis_script_writes_the_reference_files(tmp_path):
    env = dict(os.environ)
    data = str(tmp_path / "data")
    env.update({"PYTHONPATH": PKG, "KVQ_SYNTHETIC_SENTENCES": "200", "KVQ_BATCH_SIZE": "50", "KVQ_LIM_BATCHES": "2",
                "KVQ_ENCODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_DECODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_VQ_E_DIM": "128",
                "KVQ_PER_SLOT_MEAN": "True", "KVQ_SENTENCES_PATH": repr(data + "/dSentences_sentences.npy"),
                "KVQ_RESULTS_DIR": repr(str(tmp_path / "results"))})
    script = os.path.join(PKG, "analyses", "cross_attention", "extract_model_cross_attention.py")
    r = subprocess.run([sys.executable, script], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "100 sentences" in r.stdout
    out = tmp_path / "results"
    cross = torch.load(out / "cross_attentions_mean_across_batch_size.pth")
    self_ = torch.load(out / "attentions_mean_across_batch_size.pth")
    for t in (cross, self_):
        assert t.shape == (2, 2, 12, 12) and t.dtype == torch.float32
        assert float((t.sum(-1) - 1).abs().max()) <= 1e-5        # a mean of probability rows is a probability row
    assert not torch.equal(cross, self_)                         # (the reference saves the cross maps under both names)
    assert float(self_.triu(1).abs().max()) == 0.0               # decoder self-attention is causal
    for name in ("cross_attentions", "attentions"):
        slots = torch.load(out / f"{name}_mean_across_num_batches.pth")
        assert slots.shape == (2, 50, 2, 12, 12) and slots.dtype == torch.float32
    torch.testing.assert_close(torch.load(out / "cross_attentions_mean_across_num_batches.pth").mean(1), cross, rtol=0, atol=1e-6)
