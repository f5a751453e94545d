"""TrainEngine.generate / generate_codes / traverse_codes(free_running=True): the key/value-cache decoder against the existing
teacher-forced path of the same engine and against the model's own HuggingFace modules in f32.

Models: kvq-bert-tiny (2 layers, 2 heads, H = 128, V = 2048, 64 positions), built as tests/test_latent_engine_gpu.py builds them:
Shelgon with a VectorQuantizer (K = 32) -- latents = codebook rows of seeded random indices -- and Bagon -- seeded normal latents.
B = 6, Se = 12, max_length = 20, P = 1; a second case B = 3, P = 4, whose batch is padded to 8 rows with live pad rows.

The check rests on causality: decode(latents, G, ones) teacher-forced on the generated G computes at position t, from G[:, :t + 1],
the logits generation chose G[:, t + 1] from.  Tolerances:
  f32   rtol = atol = 2e-4 against HuggingFace f32 (tests/test_engine_gpu.py:335, the project's figure for f32 logits)
  bf16  E_TF = max |decode() bf16 logits - HF f32 logits| on these inputs, measured on the EXISTING path (constants below name the
        run); the cache path must stay within 2 E_TF of HF f32: another row count changes tile and summation order, not the
        precision class
Tokens are compared where the reference's answer is determined: each of the two largest logits may move by tol, so a token whose
top-2 gap is below 2 tol is left out; against HF at most 5 % of the tokens may be (a condition of the test; seed chosen on the
CPU with the HF modules alone, share in profiles/generate.md).  Between generate() and decode() of one engine the per-logit
distance is bounded by the sum of their distances to HF: tol = 2 (2e-4 + 2e-4 |x|) in f32, 3 E_TF in bf16.
"""
import functools

import pytest
import torch

from test_latent_engine_gpu import K, build, hf_modules

pytestmark = pytest.mark.gpu

B, SE, L, H, V = 6, 12, 20, 128, 2048
RTOL = ATOL = 2e-4
START = 101                              # [CLS]
SEED = 1                                 # latents / prompts; chosen on the CPU (profiles/generate.md): HF alone leaves out 1 of 114 tokens (0.9 %)
# max |decode() bf16 logits - HF f32 logits| of the EXISTING teacher-forced path on these inputs (the same at the parent commit),
# and what the cache path measured in the same run -- MI355X, run recorded in profiles/generate.md
E_TF_MEASURED = {"shelgon": 0.009577, "bagon": 0.008920}
CACHE_ERR_MEASURED = {"shelgon": 0.009577, "bagon": 0.009035}


def latents_of(kind, model, seed, n=B):
    """f32 latents [n, SE, H] on the CPU and, for Shelgon, the indices they are the codebook rows of"""
    g = torch.Generator().manual_seed(seed)
    if kind == "bagon":
        return torch.randn((n, SE, H), generator=g), None
    idx = torch.randint(0, K, (n, SE), generator=g)
    return model.vector_quantizer.embedding.weight.detach().float().cpu()[idx], idx


@functools.lru_cache(maxsize=None)
def case(kind, dtype):
    from kvq.engine import engine_of
    model = build(kind)
    ref = hf_modules(model, "cuda")
    lat32, idx = latents_of(kind, model, SEED)
    model.compute_dtype = dtype
    model = model.cuda().eval()
    eng = engine_of(model)
    assert eng.dtype == dtype
    lat = lat32.to(dtype).cuda().contiguous()
    prompt = torch.full((B, 1), START, dtype=torch.int64, device="cuda")
    fixed = tuple(t.cuda() for t in (torch.randint(1000, 2000, (B, SE), generator=torch.Generator().manual_seed(9)), torch.ones(B, SE, dtype=torch.int64)))
    with torch.no_grad():
        before = eng.forward_logits(*fixed)["logits"].clone()
        gen = eng.generate(lat, L, prompt, want_logits=True)
        after = eng.forward_logits(*fixed)["logits"].clone()
        G = gen["ids"]
        tf = eng.decode(lat, G, torch.ones_like(G), want_logits=True)["logits"].float()
        hf = ref.decoder(encoder_hidden_states=lat.float(), input_ids=G, attention_mask=torch.ones_like(G)).logits
    torch.cuda.synchronize()
    return dict(model=model, ref=ref, eng=eng, lat=lat, idx=None if idx is None else idx.cuda(), prompt=prompt, gen=gen, G=G, tf=tf, hf=hf,
                before=before, after=after)


def decided(logits, tol_of):
    """tokens whose arg-max survives a move of every logit by tol: top-2 gap above 2 tol"""
    top = logits.topk(2, dim=-1).values
    return (top[..., 0] - top[..., 1]) > 2 * tol_of(top[..., 0])


CASES = [("shelgon", torch.float32), ("shelgon", torch.bfloat16), ("bagon", torch.float32), ("bagon", torch.bfloat16)]


@pytest.mark.parametrize("kind,dtype", CASES)
def test_generated_tokens_are_the_argmax_of_the_teacher_forced_logits(kind, dtype):
    c = case(kind, dtype)
    G, tf, gen = c["G"], c["tf"], c["gen"]
    assert G.shape == (B, L) and G.dtype == torch.int64 and bool((G[:, 0] == START).all())
    assert gen["lengths"].tolist() == [L] * B and not bool(gen["finished"].any())
    assert gen["logits"].shape == (B, L - 1, V) and gen["logits"].dtype == torch.float32
    if dtype == torch.float32:
        tol_of = lambda x: 2 * (ATOL + RTOL * x.abs())
    else:
        tol_of = lambda x: torch.full_like(x, 3 * E_TF_MEASURED[kind])
    ok = decided(tf[:, :L - 1], tol_of)
    differ = (G[:, 1:] != tf[:, :L - 1].argmax(-1)) & ok
    dist = float((gen["logits"] - tf[:, :L - 1]).abs().max())
    print(f"\n[generate self-consistency {kind} {dtype}] {int(ok.sum())} of {ok.numel()} tokens decided, {int(differ.sum())} differ; "
          f"max |step logits - teacher-forced logits| = {dist:.3e}")
    # the premise of the token rule, asserted on its own: every step logit within tol of its teacher-forced twin.  (How many tokens
    # the rule then decides is a property of this untrained model's top-2 gaps, not of the code under test: printed, and not empty)
    assert bool(((gen["logits"] - tf[:, :L - 1]).abs() <= tol_of(tf[:, :L - 1])).all())
    assert bool(ok.any())
    assert int(differ.sum()) == 0
    # the choice is the arg-max of the step's own logits, always
    assert torch.equal(G[:, 1:].cpu(), gen["logits"].cpu().argmax(-1))


def test_per_layer_cross_attention_fill_with_one_frozen_key_weight():
    """One decoder layer's cross-attention key weight frozen before the engine is built: ca.k / ca.v are no longer uniformly
    trainable, so generate / beam_search fill the cross-attention keys | values with one GEMM per layer instead of one for all.
    f32, the file's own B, Se, L, P = 1; the rules of test_generated_tokens_are_the_argmax_... on that arm."""
    from kvq.engine import engine_of
    model = build("shelgon")
    lat32, _ = latents_of("shelgon", model, SEED)
    model.decoder.bert.encoder.layer[0].crossattention.self.key.weight.requires_grad_(False)
    model = model.cuda().eval()
    eng = engine_of(model)
    assert eng.dtype == torch.float32 and eng._cakv_batched is False
    lat = lat32.cuda().contiguous()
    prompt = torch.full((B, 1), START, dtype=torch.int64, device="cuda")
    with torch.no_grad():
        gen = eng.generate(lat, L, prompt, want_logits=True)
        G = gen["ids"]
        tf = eng.decode(lat, G, torch.ones_like(G), want_logits=True)["logits"].float()[:, :L - 1]
        one = eng.beam_search(lat, L, prompt, num_beams=1)
    assert G.shape == (B, L) and gen["logits"].shape == (B, L - 1, V)
    dist = (gen["logits"] - tf).abs()
    print(f"\n[generate, per-layer keys | values fill] max |step logits - teacher-forced logits| = {float(dist.max()):.3e}")
    assert bool((dist <= 2 * (ATOL + RTOL * tf.abs())).all())
    assert torch.equal(G[:, 1:].cpu(), gen["logits"].cpu().argmax(-1))
    assert torch.equal(one["ids"], G)


@pytest.mark.parametrize("kind", ["shelgon", "bagon"])
def test_f32_step_logits_against_huggingface(kind):
    c = case(kind, torch.float32)
    G, hf, got = c["G"], c["hf"][:, :L - 1], c["gen"]["logits"]
    torch.testing.assert_close(got, hf, rtol=RTOL, atol=ATOL)
    ok = decided(hf, lambda x: ATOL + RTOL * x.abs())
    left_out = 1.0 - float(ok.float().mean())
    differ = int(((G[:, 1:] != hf.argmax(-1)) & ok).sum())
    print(f"\n[generate vs HF f32 {kind}] seed {SEED}: {left_out:.4f} of {ok.numel()} tokens left out (top-2 gap below 2 tol), "
          f"{differ} decided tokens differ, {int((G[:, 1:] != hf.argmax(-1)).sum())} of all")
    assert left_out <= 0.05
    assert differ == 0


@pytest.mark.parametrize("kind", ["shelgon", "bagon"])
def test_bf16_cache_path_stays_within_twice_the_teacher_forced_error(kind):
    c = case(kind, torch.bfloat16)
    hf = c["hf"]
    e_tf = float((c["tf"] - hf).abs().max())
    e_cache = float((c["gen"]["logits"] - hf[:, :L - 1]).abs().max())
    print(f"\n[generate bf16 {kind}] e_tf = max |decode() - HF f32| = {e_tf:.6f} (recorded {E_TF_MEASURED[kind]:.6f}); "
          f"cache path max |step logits - HF f32| = {e_cache:.6f} (recorded {CACHE_ERR_MEASURED[kind]:.6f}); bound 2 e_tf = {2 * E_TF_MEASURED[kind]:.6f}")
    assert 0.5 * E_TF_MEASURED[kind] <= e_tf <= 2 * E_TF_MEASURED[kind]      # the recorded figure still describes the existing path
    assert e_cache <= 2 * E_TF_MEASURED[kind]
    ok = decided(hf[:, :L - 1], lambda x: torch.full_like(x, 2 * E_TF_MEASURED[kind]))
    assert int(((c["G"][:, 1:] != hf[:, :L - 1].argmax(-1)) & ok).sum()) == 0


@pytest.mark.parametrize("kind,dtype", CASES)
def test_graph_and_eager_steps_agree_bit_for_bit_and_the_graph_is_reused(kind, dtype):
    c = case(kind, dtype)
    eng = c["eng"]
    entry = next(g for g in eng._gen_cache.values() if g["B"] == B and g["step_logits"] is not None)
    graph, replays = entry["graph"], entry["replays"]
    assert graph is not None and replays >= L - 1
    with torch.no_grad():
        eager = eng.generate(c["lat"], L, c["prompt"], want_logits=True, graph=False)
        assert entry["replays"] == replays
        again = eng.generate(c["lat"], L, c["prompt"], want_logits=True)
    assert entry["graph"] is graph and entry["replays"] == replays + L - 1          # the second call replays the first call's graph
    for k in ("ids", "logits", "lengths", "finished"):
        assert torch.equal(eager[k], c["gen"][k]), k
        assert torch.equal(again[k], c["gen"][k]), k
    census = eng.gen_census()
    assert census, "no captured generation step"
    for n in census:
        assert n["kernel"] > 0 and n["memset"] == 0 and n["memcpy"] == 0 and n["empty"] == 0 and n["event"] == 0 and n["other"] == 0, n
    assert torch.equal(c["before"], c["after"])                                     # forward_logits: the same bits around a generate call


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pad_rows_never_show_and_do_not_reach_the_live_rows(dtype):
    """B = 3 (five pad rows) with a prompt of P = 4 against the same three sentences inside B = 8 (no pad row)"""
    c = case("shelgon", dtype)
    eng = c["eng"]
    lat8 = latents_of("shelgon", c["model"], 5, n=8)[0].to(dtype).cuda().contiguous()
    prompt8 = torch.randint(1000, 2000, (8, 4), generator=torch.Generator().manual_seed(6)).cuda()
    prompt8[:, 0] = START
    with torch.no_grad():
        small = eng.generate(lat8[:3].contiguous(), L, prompt8[:3].contiguous(), want_logits=True)
        big = eng.generate(lat8, L, prompt8, want_logits=True)
        tf = eng.decode(lat8[:3].contiguous(), small["ids"], torch.ones_like(small["ids"]), want_logits=True)["logits"].float()
    assert small["ids"].shape == (3, L) and small["logits"].shape == (3, L - 1, V) and small["lengths"].shape == (3,) and small["finished"].shape == (3,)
    assert torch.equal(small["ids"][:, :4], prompt8[:3])                            # the prompt is kept
    for k in ("ids", "logits", "lengths", "finished"):
        assert torch.equal(small[k], big[k][:3]), k
    # prompt positions went through the same step path: their logits are the teacher-forced ones too
    tol_of = (lambda x: 2 * (ATOL + RTOL * x.abs())) if dtype == torch.float32 else (lambda x: torch.full_like(x, 3 * E_TF_MEASURED["shelgon"]))
    ok = decided(tf[:, 3:L - 1], tol_of)
    assert int(((small["ids"][:, 4:] != tf[:, 3:L - 1].argmax(-1)) & ok).sum()) == 0 and bool(ok.any())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_end_token_finishes_a_sentence_and_pads_follow(dtype):
    c = case("bagon", dtype)
    eng, G = c["eng"], c["G"]
    eos, pad = int(G[0, 5]), 7                                                     # a token greedy generation is seen to emit
    with torch.no_grad():
        out = eng.generate(c["lat"], L, c["prompt"], eos_id=eos, pad_id=pad)
    assert "logits" not in out
    hits = 0
    for b in range(B):
        where = (G[b, 1:] == eos).nonzero()
        if len(where):
            n = int(where[0]) + 2                                                  # tokens up to and including the end token
            hits += 1
            assert bool(out["finished"][b]) and int(out["lengths"][b]) == n
            assert torch.equal(out["ids"][b, :n], G[b, :n]) and bool((out["ids"][b, n:] == pad).all())
        else:
            assert not bool(out["finished"][b]) and int(out["lengths"][b]) == L and torch.equal(out["ids"][b], G[b])
    assert hits >= 1 and int(out["lengths"][0]) <= 6


def test_generate_codes_and_free_running_traversal_are_generate_of_the_codebook_rows():
    for dtype in (torch.float32, torch.bfloat16):
        c = case("shelgon", dtype)
        eng, idx = c["eng"], c["idx"]
        with torch.no_grad():
            assert torch.equal(eng.codes_to_latents(idx), c["lat"])
            a = eng.generate_codes(idx, L, c["prompt"], want_logits=True)
            for k in ("ids", "logits", "lengths", "finished"):
                assert torch.equal(a[k], c["gen"][k]), k
            assert torch.equal(c["model"].generate_from_codes(idx, L, c["prompt"])["ids"], c["G"])
            e = torch.randint(1000, 2000, (B, SE), generator=torch.Generator().manual_seed(11)).cuda()
            em = torch.ones_like(e)
            tr = eng.traverse_codes(e, em, 2, 3, free_running=True, max_length=L, start_id=START)
            own = eng.encode(e, em)["indices"].reshape(B, SE, 1)[2]
            rows = own.unsqueeze(0).repeat(K, 1, 1)
            rows[:, 3, 0] = torch.arange(K, device="cuda")
            want = eng.generate_codes(rows, L, torch.full((K, 1), START, dtype=torch.int64, device="cuda"))["ids"]
        assert tr["recon_ids"].shape == (K, L) and torch.equal(tr["recon_ids"], want)
        assert tr["own_code"] == int(own[3, 0]) and torch.equal(tr["changed"], want != want[tr["own_code"]].unsqueeze(0))
        teacher = eng.traverse_codes(e, em, 2, 3)                                   # the default is the teacher-forced traversal, as before
        assert teacher["recon_ids"].shape == (K, SE)


def test_sampling_repeats_under_one_seed_and_differs_under_another():
    c = case("bagon", torch.bfloat16)
    eng = c["eng"]
    with torch.no_grad():
        assert torch.equal(eng.generate(c["lat"], L, c["prompt"])["ids"], c["G"])
        entries = dict(eng._gen_cache)
        entry = next(g for g in entries.values() if g["B"] == B and g["step_logits"] is None)
        graph, replays = entry["graph"], entry["replays"]
        a = eng.generate(c["lat"], L, c["prompt"], temperature=1.0, seed=3)
        b = eng.generate(c["lat"], L, c["prompt"], temperature=1.0, seed=3)
        d = eng.generate(c["lat"], L, c["prompt"], temperature=1.0, seed=4)
        f = eng.generate(c["lat"], L, c["prompt"], temperature=0.5, seed=(1 << 40) + 3)
        # temperature and seed live in the device state: no new buffers, the greedy call's captured step serves them all
        assert dict(eng._gen_cache) == entries and entry["graph"] is graph and entry["replays"] == replays + 4 * (L - 1)
        e = eng.generate(c["lat"], L, c["prompt"], temperature=1.0, seed=3, graph=False)
    assert not torch.equal(f["ids"], a["ids"])
    assert torch.equal(a["ids"], b["ids"]) and torch.equal(a["ids"], e["ids"]) and not torch.equal(a["ids"], d["ids"])
    assert not torch.equal(a["ids"], c["G"])
    bm = c["model"]
    assert torch.equal(bm.generate_from_latents(c["lat"], L, c["prompt"])["ids"], c["G"])


def test_refusals_happen_before_any_launch_and_an_ordinary_call_follows():
    from kvq._ffi import KvqError
    c = case("shelgon", torch.float32)
    eng, lat, prompt = c["eng"], c["lat"], c["prompt"]
    calls = {"generate": lambda: eng.generate(lat, L, prompt), "generate_codes": lambda: eng.generate_codes(c["idx"], L, prompt)}
    for attr, value, text in (("_cap", object(), "graph capture"), ("group", object(), "process group"), ("fp8", True, "fp8")):
        old = getattr(eng, attr)
        setattr(eng, attr, value)
        try:
            for name, fn in calls.items():
                with pytest.raises(KvqError, match=text):
                    fn()
        finally:
            setattr(eng, attr, old)
    with pytest.raises(KvqError, match="sequence length"):                         # f32 ends at 32 tokens
        eng.generate(lat, 40, prompt)
    with pytest.raises(KvqError, match="sequence length"):
        eng.generate(torch.zeros(B, 40, H, device="cuda"), L, prompt)
    with pytest.raises(KvqError, match="position table"):
        eng.generate(lat, 65, prompt)
    beng = case("shelgon", torch.bfloat16)["eng"]
    with pytest.raises(KvqError, match="position table"):                          # inside bf16's 128 tokens, outside the 64 positions
        beng.generate(lat.bfloat16(), 100, prompt)
    with pytest.raises(KvqError, match="latents must be"):
        eng.generate(lat[:, :, :64].contiguous(), L, prompt)                       # wrong H
    with pytest.raises(KvqError, match="contiguous"):
        eng.generate(lat.bfloat16(), L, prompt)                                    # not the engine's dtype
    with pytest.raises(KvqError, match="contiguous"):
        eng.generate(lat.cpu(), L, prompt)                                         # not on the device
    with pytest.raises(KvqError, match="contiguous"):
        eng.generate(lat[:, ::2], L, prompt)                                      # not contiguous
    with pytest.raises(KvqError, match="prompt_ids must be"):
        eng.generate(lat, L, prompt[:4])                                           # another batch size
    with pytest.raises(KvqError, match="prompt_ids must be"):
        eng.generate(lat, L, prompt.int())
    with pytest.raises(KvqError, match="prompt_ids must be"):
        eng.generate(lat, L, prompt.view(-1))
    with pytest.raises(KvqError, match="prompt_ids must be on"):
        eng.generate(lat, L, prompt.cpu())
    with pytest.raises(KvqError, match="does not fit"):
        eng.generate(lat, 3, torch.full((B, 4), START, dtype=torch.int64, device="cuda"))
    with pytest.raises(KvqError, match="temperature"):
        eng.generate(lat, L, prompt, temperature=-1.0)
    for kw, text in ((dict(eos_id=True), "eos_id"), (dict(eos_id=V), "eos_id"), (dict(eos_id=1.0), "eos_id"), (dict(pad_id=-1), "pad_id"),
                     (dict(pad_id=V), "pad_id"), (dict(seed=-1), "seed"), (dict(seed=1.5), "seed"), (dict(seed=1 << 64), "seed")):
        with pytest.raises(KvqError, match=text):
            eng.generate(lat, L, prompt, **kw)
        with pytest.raises(KvqError, match=text):
            eng.generate_codes(c["idx"], L, prompt, **kw)
    bad_prompt = prompt.clone()
    bad_prompt[3, 0] = V
    with pytest.raises(KvqError, match="prompt_ids hold ids outside"):
        eng.generate(lat, L, bad_prompt)
    bad_prompt[3, 0] = -1
    with pytest.raises(KvqError, match="prompt_ids hold ids outside"):
        eng.generate_codes(c["idx"], L, bad_prompt)
    with pytest.raises(KvqError, match="no quantiser"):
        case("bagon", torch.float32)["eng"].generate(case("bagon", torch.float32)["lat"], L, prompt, quantize=True)
    with torch.no_grad():
        q = eng.generate(lat, L, prompt, quantize=True)                            # codebook rows quantise to themselves
        assert torch.equal(q["indices"].reshape(B, SE), c["idx"]) and torch.equal(q["ids"], c["G"])
        assert torch.equal(eng.generate(lat, L, prompt)["ids"], c["G"])


def _run_analysis(script, tmp_path, args=(), **overrides):
    import os
    import subprocess
    import sys
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kindergarten-vq-vae_amd")
    env = dict(os.environ)
    env.update({"PYTHONPATH": pkg, "KVQ_SYNTHETIC_SENTENCES": "200", "KVQ_BATCH_SIZE": "50",
                "KVQ_ENCODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_DECODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_VQ_E_DIM": "128",
                "KVQ_SENTENCES_PATH": repr(str(tmp_path / "data" / "dSentences_sentences.npy")),
                "KVQ_LATENT_CLASSES_LABELS_PATH": repr(str(tmp_path / "data" / "dSentences_latent_classes_labels.npy")),
                "KVQ_RUN_DIR": repr(str(tmp_path / "run"))})
    env.update(overrides)
    r = subprocess.run([sys.executable, os.path.join(pkg, "analyses", *script), *args], env=env, cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_code_traversal_script_takes_the_free_running_switch(tmp_path):
    """the command-line form of the switch; the table keeps its shape"""
    from analyses.get_max_acc_sentences import read_table
    out = _run_analysis(("latent_traversals", "code_traversal.py"), tmp_path, args=("--free-running",), KVQ_POSITIONS="[2]", KVQ_VQ_N_E="9")
    assert "variants" in out
    df = read_table(str(tmp_path / "run" / "code_traversal.feather"))
    assert len(df) == 9 and sorted(set(df["code"])) == list(range(9))
    own = df[df["own_code"]]
    assert len(own) == 1 and int(own["n_changed_tokens"].iloc[0]) == 0


def test_latent_arithmetics_script_takes_the_free_running_constant(tmp_path):
    """the configuration form of the switch (KVQ_FREE_RUNNING); the table keeps its shape"""
    from analyses.get_max_acc_sentences import read_table
    out = _run_analysis(("latent_arithmetics", "latent_arithmetics.py"), tmp_path, KVQ_MODEL_NAME="'Bagon'", KVQ_N_SENTENCES="20",
                        KVQ_FREE_RUNNING="True")
    assert "edited" in out
    df = read_table(str(tmp_path / "run" / "latent_arithmetics.feather"))
    assert list(df.columns) == ["input_sentence", "recon_sentence", "edited_sentence"] and len(df) == 20
