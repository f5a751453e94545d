"""TrainEngine.encode / decode / decode_codes / traverse_codes and kvq.census.LatentCensus on the engine's kernels.

Models: kvq-bert-tiny (2 layers, 2 heads, H = 128), B = 6: Shelgon with a VectorQuantizer (K = 32) on the autoencoding call
(S = 12), Shelgon with a MultiVectorQuantizer (2 codebooks of 32 x 64), and Bagon with decoder ids != encoder ids and a decoder
length (10) other than the encoder's (12).
References: the existing path of the same engine (bitwise: same kernels, same inputs), and the model's own HuggingFace modules in
f32.  Tolerance against HF: rtol = atol = 2e-4, what tests/test_engine_gpu.py::test_hf_forward_kvq_path_and_engine_agree_on_gpu
applies to f32 logits of the whole forward.
Arg-max ids against HF are compared where HF's own answer is determined under that tolerance: each of the two largest logits may
move by tol = 2e-4 + 2e-4 |logit|, so a token whose top-2 gap is below 2 tol is left out; at most 5 % of the tokens may be (a
condition of the test; seed and measured share: profiles/latent_analyses.md).
"""
import copy
import functools
import os
import subprocess
import sys

import pytest
import torch

import _latent_ref as R
from _gemm_guard import forbid_vendor_gemms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")

B, S, SD, K = 6, 12, 10, 32
RTOL = ATOL = 2e-4                      # tests/test_engine_gpu.py:335
ARITH_SEED = 1                          # batches of the end-to-end arithmetic (chosen on the CPU, see arithmetic_hf)


def build(kind):
    from models.bagon.Bagon import Bagon
    from models.shelgon3.MultiVectorQuantizer import MultiVectorQuantizer
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(0)
    if kind == "bagon":
        return Bagon("kvq-bert-tiny", "kvq-bert-tiny", True, compute_dtype=torch.float32)
    if kind == "multi":
        vq = MultiVectorQuantizer(2, K, 128, 0.25)
        with torch.no_grad():
            vq.embedding.weight.copy_(torch.randn(2 * K, 64))
    else:
        vq = VectorQuantizer(K, 128, 0.25, vq_codebook_init_values=torch.randn(K, 128))
        vq.materialize_min_encodings = False
    return Shelgon("kvq-bert-tiny", vq, "kvq-bert-tiny", None, compute_dtype=torch.float32)


def batch(kind, seed, device="cuda"):
    """(enc ids, enc mask, dec ids, dec mask): Shelgon decodes the encoder's ids; Bagon other ids of another length"""
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(3, S + 1, (B,), generator=g)
    keep = torch.arange(S)[None] < lens[:, None]
    e = torch.randint(1000, 2000, (B, S), generator=g) * keep
    em = keep.long()
    if kind != "bagon":
        return tuple(t.to(device) for t in (e, em, e, em))
    dkeep = torch.arange(SD)[None] < lens.clamp(max=SD)[:, None]
    d = torch.randint(1000, 2000, (B, SD), generator=g) * dkeep
    return tuple(t.to(device) for t in (e, em, d, dkeep.long()))


def hf_modules(model, device):
    ref = copy.deepcopy(model).to(device).eval()
    for m in (ref.encoder, ref.decoder):
        m.set_attn_implementation("eager")
    return ref


@functools.lru_cache(maxsize=None)
def case(kind, dtype):
    from kvq.engine import engine_of
    model = build(kind)
    ref = hf_modules(model, "cuda") if dtype == torch.float32 else None
    model.compute_dtype = dtype
    model = model.cuda().eval()
    eng = engine_of(model)
    assert eng.dtype == dtype
    b = batch(kind, 1)
    with torch.no_grad():
        before = eng.forward_logits(*b)
        enc = eng.encode(b[0], b[1])
        src = enc["z_q"] if kind != "bagon" else enc["z"]
        dec = eng.decode(src, b[2], b[3], want_logits=True)
        after = eng.forward_logits(*b)
    torch.cuda.synchronize()
    return dict(model=model, ref=ref, eng=eng, batch=b, before=before, enc=enc, dec=dec, after=after)


BITS = [("shelgon", torch.float32), ("shelgon", torch.bfloat16), ("bagon", torch.float32), ("multi", torch.bfloat16)]


@pytest.mark.parametrize("kind,dtype", BITS)
def test_decode_of_the_encoded_latent_has_the_bits_of_forward_logits(kind, dtype):
    c = case(kind, dtype)
    eng, (e, em, d, dm), fl = c["eng"], c["batch"], c["before"]
    assert c["enc"]["z"].shape == (B, S, 128) and c["enc"]["z"].dtype == dtype
    assert c["dec"]["logits"].shape == fl["logits"].shape and torch.equal(c["dec"]["logits"], fl["logits"])
    for k in ("recon_ids", "acc", "loss_recon"):
        assert torch.equal(c["dec"][k], fl[k]), k
    want_acc = (fl["recon_ids"] == d).float().mean(1)
    assert c["dec"]["acc_per_sentence"].shape == (B,) and float((c["dec"]["acc_per_sentence"] - want_acc).abs().max()) <= 1e-6
    if kind == "bagon":
        assert set(c["enc"]) == {"z"}
        return
    with torch.no_grad():
        q = eng.decode(c["enc"]["z"], d, dm, quantize=True, want_logits=True)
        plain = eng.encode(e, em, quantize=False)
    assert torch.equal(q["logits"], fl["logits"]) and torch.equal(q["indices"], fl["indices"])
    assert set(plain) == {"z"} and torch.equal(plain["z"], c["enc"]["z"])
    assert c["enc"]["indices"].shape == fl["indices"].shape and torch.equal(c["enc"]["indices"], eng.code_indices(e, em)["indices"])
    assert torch.equal(c["enc"]["indices"], fl["indices"])
    assert torch.equal(c["enc"]["perplexity"], fl["perplexity"]) and torch.equal(c["enc"]["loss_vq_raw"], fl["loss_vq_raw"])


@pytest.mark.parametrize("kind,dtype", BITS)
def test_forward_logits_bits_do_not_move(kind, dtype):
    c = case(kind, dtype)
    assert torch.equal(c["before"]["logits"], c["after"]["logits"]) and c["eng"]._maps is None


@pytest.mark.parametrize("kind", ["shelgon", "bagon"])
def test_encode_and_decode_of_an_edited_latent_against_huggingface_f32(kind):
    c = case(kind, torch.float32)
    eng, ref, (e, em, d, dm) = c["eng"], c["ref"], c["batch"]
    with torch.no_grad():
        z_hf = ref.encoder(e, attention_mask=em).last_hidden_state
        torch.testing.assert_close(c["enc"]["z"], z_hf, rtol=RTOL, atol=ATOL)
        edited = (z_hf + 0.5 * torch.randn(z_hf.shape, generator=torch.Generator().manual_seed(3)).cuda()).contiguous()
        want = ref.decoder(encoder_hidden_states=edited, input_ids=d, attention_mask=dm).logits
        got = eng.decode(edited, d, dm, want_logits=True)
    torch.testing.assert_close(got["logits"], want, rtol=RTOL, atol=ATOL)
    assert not torch.allclose(want, c["before"]["logits"], rtol=RTOL, atol=10 * ATOL)          # the edit is visible at this tolerance
    tgt = torch.randint(1000, 2000, d.shape, generator=torch.Generator().manual_seed(4)).cuda()
    with torch.no_grad():
        scored = eng.decode(edited, d, dm, target_ids=tgt)
    assert torch.equal(scored["recon_ids"], got["recon_ids"]) and "logits" not in scored
    want_loss = torch.nn.functional.cross_entropy(want.reshape(-1, want.shape[-1]), tgt.reshape(-1))
    assert abs(float(scored["loss_recon"]) - float(want_loss)) <= 2e-5 * float(want_loss)     # tests/test_engine_gpu.py:340


@pytest.mark.parametrize("kind", ["shelgon", "multi"])
def test_decode_codes_against_huggingface_on_the_codebook_rows(kind):
    c = case(kind, torch.float32)
    eng, ref, (e, em, d, dm) = c["eng"], c["ref"], c["batch"]
    G = 1 if kind == "shelgon" else 2
    idx = torch.randint(0, K, (B, S, G), generator=torch.Generator().manual_seed(5)).cuda()
    E = ref.vector_quantizer.embedding.weight
    rows = R.lookup_ref(E, idx.view(-1, G), K, torch.float32).view(B, S, 128)
    with torch.no_grad():
        assert torch.equal(eng.codes_to_latents(idx), rows)
        want = ref.decoder(encoder_hidden_states=rows, input_ids=d, attention_mask=dm).logits
        got = eng.decode_codes(idx, d, dm, want_logits=True)
        if G == 1:
            assert torch.equal(eng.decode_codes(idx[:, :, 0], d, dm, want_logits=True)["logits"], got["logits"])
    torch.testing.assert_close(got["logits"], want, rtol=RTOL, atol=ATOL)


def arithmetic_hf(ref, device):
    """The end-to-end arithmetic with HF modules and torch f64 means: three batches of labelled sentences (groups 0 / 1, some left
    out), direction = mean(1) - mean(0), added to the first batch's encoder outputs, decoded with that batch's decoder input.
    -> (batches, labels, HF arg-max ids [B, Sd], mask of tokens whose top-2 gap is at least 2 tol)"""
    batches = [batch("bagon", ARITH_SEED + i, device) for i in range(3)]
    labels = [torch.tensor([(0, 1, 1, -1, 0, 1)[(i + j) % 6] for i in range(B)]) for j in range(3)]
    with torch.no_grad():
        zs = [ref.encoder(b[0], attention_mask=b[1]).last_hidden_state for b in batches]
        direction = R.mean_direction_ref(torch.cat(zs), torch.cat(labels), 1, 0)
        edited = (zs[0].double() + direction).float()
        logits = ref.decoder(encoder_hidden_states=edited, input_ids=batches[0][2], attention_mask=batches[0][3]).logits
    top = logits.topk(2, dim=-1).values
    tol = ATOL + RTOL * top[..., 0].abs()
    return batches, labels, logits.argmax(-1), (top[..., 0] - top[..., 1]) >= 2 * tol


def test_latent_arithmetic_end_to_end_against_huggingface():
    from kvq.census import LatentCensus
    c = case("bagon", torch.float32)
    eng = c["eng"]
    batches, labels, ids_hf, decided = arithmetic_hf(c["ref"], "cuda")
    left_out = 1.0 - float(decided.float().mean())
    census = LatentCensus(2, S, 128)
    with torch.no_grad():
        zs = [eng.encode(b[0], b[1])["z"] for b in batches]
        for z, lab in zip(zs, labels):
            census.add(z, lab)
        got = eng.decode(census.shift(zs[0], 1, 0), batches[0][2], batches[0][3])
    assert census.results()["count"].tolist() == [sum(int((l == g).sum()) for l in labels) for g in (0, 1)]
    differ = int(((got["recon_ids"] != ids_hf) & decided).sum())
    print(f"\n[latent arithmetic] seed {ARITH_SEED}: {left_out:.4f} of {decided.numel()} tokens left out (top-2 gap below 2 tol), "
          f"{differ} decided tokens differ, {int((got['recon_ids'] != ids_hf).sum())} of all")
    assert left_out <= 0.05
    assert differ == 0


@pytest.mark.parametrize("kind,dtype,factor", [("shelgon", torch.float32, 0), ("shelgon", torch.bfloat16, 0), ("multi", torch.bfloat16, 1)])
def test_traverse_codes_equals_decode_codes_on_hand_built_rows(kind, dtype, factor):
    c = case(kind, dtype)
    eng, (e, em, d, dm) = c["eng"], c["batch"]
    sentence, position = 2, 1
    with torch.no_grad():
        out = eng.traverse_codes(e, em, sentence, position, factor=factor)
        own = c["enc"]["indices"].reshape(B, S, -1)[sentence]
        rows = own.unsqueeze(0).repeat(K, 1, 1)
        for k in range(K):
            rows[k, position, factor] = k
        want = eng.decode_codes(rows, e[sentence].repeat(K, 1), em[sentence].repeat(K, 1))["recon_ids"]
    assert out["recon_ids"].shape == (K, S) and torch.equal(out["recon_ids"], want)
    assert out["own_code"] == int(own[position, factor]) and out["changed"].dtype == torch.bool
    assert not bool(out["changed"][out["own_code"]].any())
    assert torch.equal(out["changed"], want != want[out["own_code"]])
    via_model = c["model"].traverse_codes(e, em, sentence, position, factor=factor)
    assert torch.equal(via_model["recon_ids"], want)


@pytest.mark.parametrize("kind", ["shelgon", "multi", "bagon"])
def test_bf16_product_path_runs_without_vendor_gemms_and_repeats_bit_for_bit(kind, monkeypatch):
    from kvq.census import LatentCensus
    c = case(kind, torch.bfloat16)
    model, (e, em, d, dm) = c["model"], c["batch"]
    lab = torch.tensor([0, 1, 1, -1, 0, 1])
    runs = []
    with monkeypatch.context() as mp:
        forbid_vendor_gemms(mp)
        for _ in range(2):
            with torch.no_grad():
                z = model.encode_latents(e, em, quantize=False)["z"]
                census = LatentCensus(2, S, 128)
                census.add(z, lab)
                shifted = census.shift(z, 1, 0, alpha=2.0)
                out = model.decode_latents(shifted, d, dm, quantize=kind != "bagon", want_logits=True)
                res = [z, census.table, shifted, out["logits"], out["recon_ids"]]
                if kind != "bagon":
                    res.append(model.traverse_codes(e, em, 0, 0, factor=1 if kind == "multi" else 0)["recon_ids"])
            torch.cuda.synchronize()
            runs.append(res)
    assert runs[0][0].dtype == torch.bfloat16 and not torch.equal(runs[0][2], runs[0][0])
    for a, b2 in zip(*runs):
        assert torch.equal(a, b2)


def test_step_graph_is_unchanged_by_the_latent_calls():
    from kvq.census import LatentCensus
    from kvq.engine import TrainEngine
    model = build("shelgon")
    model.compute_dtype = torch.bfloat16
    model = model.cuda().train()
    eng = TrainEngine(model, lr=1e-3)
    e, em, _, _ = batch("shelgon", 4)
    for _ in range(5):
        eng.train_step(e, em)
    torch.cuda.synchronize()
    assert eng._graphs, "the step was not captured"
    keys = list(eng._graphs)
    before = [g.node_census() for g in eng._graphs.values()]
    enc = eng.encode(e, em)
    census = LatentCensus(2, S, 128)
    census.add(enc["z"], 0)
    census.add(enc["z"].flip(0), 1)
    dec = eng.decode(census.shift(enc["z"], 1, 0), e, em, quantize=True)
    trav = eng.traverse_codes(e, em, 0, 0)
    out = eng.train_step(e, em)
    torch.cuda.synchronize()
    assert list(eng._graphs) == keys and [g.node_census() for g in eng._graphs.values()] == before
    assert torch.isfinite(out["loss_recon"]) and dec["recon_ids"].shape == (B, S) and trav["recon_ids"].shape == (K, S)
    assert model.training                                       # evaluation passes; they leave the module's mode alone


def test_refusals_and_an_ordinary_call_afterwards():
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    c = case("shelgon", torch.float32)
    eng, (e, em, d, dm) = c["eng"], c["batch"]
    z = c["enc"]["z"]
    idx = c["enc"]["indices"]
    calls = {"encode": lambda: eng.encode(e, em), "decode": lambda: eng.decode(z, d, dm), "decode_codes": lambda: eng.decode_codes(idx, d, dm),
             "traverse_codes": lambda: eng.traverse_codes(e, em, 0, 0)}
    for attr, value, text in (("_cap", object(), "graph capture"), ("group", object(), "process group"), ("fp8", True, "fp8")):
        old = getattr(eng, attr)
        setattr(eng, attr, value)
        try:
            for name, fn in calls.items():
                with pytest.raises(KvqError, match=text):
                    fn()
        finally:
            setattr(eng, attr, old)
    with pytest.raises(KvqError, match="latents must be"):
        eng.decode(z[:, :, :64].contiguous(), d, dm)                     # wrong H
    with pytest.raises(KvqError, match="latents but dec_ids"):
        eng.decode(z[:4].contiguous(), d, dm)                            # batch mismatch
    with pytest.raises(KvqError, match="contiguous"):
        eng.decode(z.bfloat16(), d, dm)                                  # not the engine's dtype
    with pytest.raises(KvqError, match="dec_mask"):
        eng.decode(z, d, dm[:, :5])
    long_ids = torch.randint(1000, 2000, (B, 40), device="cuda")
    with pytest.raises(KvqError, match="sequence length"):               # f32 ends at 32 tokens
        eng.decode(z, long_ids, torch.ones_like(long_ids))
    with pytest.raises(KvqError, match="sequence length"):
        eng.encode(long_ids, torch.ones_like(long_ids))
    with pytest.raises(KvqError, match="sequence length"):
        eng.decode(torch.zeros(B, 40, 128, device="cuda"), d, dm)
    with pytest.raises(KvqError, match="indices must be"):
        eng.decode_codes(idx.reshape(B, S, 1).expand(B, S, 2), d, dm)
    bad = idx.contiguous().clone()
    bad.view(-1)[7] = K
    with pytest.raises(KvqError, match="outside"):
        eng.decode_codes(bad, d, dm)
    with pytest.raises(KvqError, match="outside"):
        eng.traverse_codes(e, em, B, 0)
    bagon = case("bagon", torch.float32)
    beng, (be, bem, bd, bdm) = bagon["eng"], bagon["batch"]
    with pytest.raises(KvqError, match="no quantiser"):
        beng.decode(bagon["enc"]["z"], bd, bdm, quantize=True)
    with pytest.raises(KvqError, match="no quantiser"):
        beng.decode_codes(torch.zeros(B, S, dtype=torch.int64, device="cuda"), bd, bdm)
    with pytest.raises(KvqError, match="no quantiser"):
        beng.traverse_codes(be, bem, 0, 0)
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    vq = VectorQuantizer(512, 768, 0.25, vq_codebook_init_values=torch.randn(512, 768))       # the model of tests/test_fp8_gpu.py
    vq.materialize_min_encodings = False
    fp8_model = Shelgon("kvq-bert-base-2l", vq, "kvq-bert-base-2l", None, compute_dtype=torch.bfloat16).cuda().eval()
    fp8_eng = TrainEngine(fp8_model, fp8_forward=True)
    with pytest.raises(KvqError, match="producer-written"):
        fp8_eng.encode(e, em)
    with pytest.raises(KvqError, match="producer-written"):
        fp8_eng.decode(torch.zeros(B, S, 768, dtype=torch.bfloat16, device="cuda"), d, dm)
    with pytest.raises(KvqError, match="producer-written"):
        fp8_eng.decode_codes(idx, d, dm)
    with torch.no_grad():                                               # and the engines go on as before
        assert torch.equal(eng.forward_logits(e, em)["logits"], c["before"]["logits"])
        assert torch.equal(eng.decode(c["enc"]["z_q"], d, dm, want_logits=True)["logits"], c["before"]["logits"])
        assert torch.equal(beng.forward_logits(be, bem, bd, bdm)["logits"], bagon["before"]["logits"])


def _run_script(script, tmp_path, **overrides):
    env = dict(os.environ)
    env.update({"PYTHONPATH": PKG, "KVQ_SYNTHETIC_SENTENCES": "200", "KVQ_BATCH_SIZE": "50",
                "KVQ_ENCODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_DECODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_VQ_E_DIM": "128",
                "KVQ_SENTENCES_PATH": repr(str(tmp_path / "data" / "dSentences_sentences.npy")),
                "KVQ_LATENT_CLASSES_LABELS_PATH": repr(str(tmp_path / "data" / "dSentences_latent_classes_labels.npy")),
                "KVQ_RUN_DIR": repr(str(tmp_path / "run"))})
    env.update(overrides)
    r = subprocess.run([sys.executable, os.path.join(PKG, "analyses", *script)], env=env, cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("model_name", ["Bagon", "Shelgon"])
def test_latent_arithmetics_script_writes_its_table(tmp_path, model_name):
    from analyses.get_max_acc_sentences import read_table
    out = _run_script(("latent_arithmetics", "latent_arithmetics.py"), tmp_path, KVQ_MODEL_NAME=repr(model_name), KVQ_N_SENTENCES="20")
    assert "edited" in out
    df = read_table(str(tmp_path / "run" / "latent_arithmetics.feather"))
    assert list(df.columns) == ["input_sentence", "recon_sentence", "edited_sentence"] and len(df) == 20
    assert all(isinstance(s, str) and s for s in df["edited_sentence"])


def test_code_traversal_script_writes_its_table(tmp_path):
    from analyses.get_max_acc_sentences import read_table
    out = _run_script(("latent_traversals", "code_traversal.py"), tmp_path, KVQ_POSITIONS="[0, 2]", KVQ_VQ_N_E="9")
    assert "variants" in out
    df = read_table(str(tmp_path / "run" / "code_traversal.feather"))
    assert len(df) == 2 * 9 and sorted(set(df["position"])) == [0, 2] and sorted(set(df["code"])) == list(range(9))
    for pos in (0, 2):
        own = df[(df["position"] == pos) & df["own_code"]]
        assert len(own) == 1 and int(own["n_changed_tokens"].iloc[0]) == 0
    assert df["input_sentence"].nunique() == 1


def test_get_max_acc_sentences_script_keeps_exactly_the_perfect_rows(tmp_path):
    import pandas as pd
    from analyses.get_max_acc_sentences import read_table, write_table
    from dsentences.synthetic import make_corpus
    sentences, _, _ = make_corpus(60, seed=3)
    acc = [1.0 if i % 3 == 0 else (0.999 if i % 3 == 1 else 11 / 12) for i in range(60)]
    df = pd.DataFrame({"epoch": 1, "stage": "test", "input_sentence": sentences.tolist(), "recon_sentence": sentences.tolist(),
                       "sentence_acc": acc})
    os.makedirs(tmp_path / "run")
    write_table(df, str(tmp_path / "run" / "decoded_sentences.feather"))
    out = _run_script(("get_max_acc_sentences.py",), tmp_path)
    assert "20 sentences" in out
    kept = read_table(str(tmp_path / "run" / "decoded_sentences_max_acc_only.feather"))
    want = sorted(s for s, a in zip(sentences.tolist(), acc) if a > 0.999)
    assert kept["input_sentence"].tolist() == want and bool((kept["sentence_acc"] > 0.999).all())
    assert os.path.getsize(tmp_path / "run" / "decoded_sentences_max_acc_only.md") > 0
