"""TrainEngine.generate(top_k, top_p, want_scores) and what passes them through, on the tiny engines of tests/_sample_case.py.

The filtered step is judged on its OWN step logits (want_logits): y = fl32(logit / temperature) formed on the CPU is the kernel's
product exactly, so the f64 reference of tests/_sample_ref.py applies row by row -- every chosen token must lie inside the largest
set the derived band allows, `kept` inside the band, token_logprobs within the derived bound, scores their f64 sum over the positions
that chose a token.  Filters off is today's call: the same bits, the same cache entries, the same graph.
"""
import os
import subprocess
import sys

import pytest
import torch

import _sample_ref as S
from _sample_case import B, K, L, SE, START, V, case, latents_of

pytestmark = pytest.mark.gpu

CASES = [("shelgon", torch.bfloat16), ("bagon", torch.float32)]


def judge(out, tau, k, p, P=1):
    """every step of a generate(want_logits=True, want_scores=True) result against the reference on its own step logits"""
    ids, lengths = out["ids"].cpu(), out["lengths"].cpu()
    n = ids.shape[0]
    total, total_bound = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(L - 1):
        y = S.y_of(out["logits"][:, t], tau)
        ref = S.Cut(y, k, p, greedy=not tau > 0)
        lo, hi = ref.keep_band()
        kept = out["kept"][:, t].cpu()
        assert bool((lo <= kept).all()) and bool((kept <= hi).all()), (t, lo, kept, hi)
        chose = (t + 1 >= P) & (t + 1 < lengths)
        tok = ids[:, t + 1]
        rank = ref.rank.gather(1, tok.unsqueeze(1)).squeeze(1)
        assert bool((rank < kept)[chose].all()) and bool((rank < hi)[chose].all()), (t, rank, kept)
        if "token_logprobs" in out:
            lp, bound = ref.logprob(tok, kept)
            err = (out["token_logprobs"][:, t].cpu().double() - lp).abs()
            assert bool((err <= bound)[chose].all()), (t, err, bound)
            total += torch.where(chose, lp, torch.zeros_like(lp))
            total_bound += torch.where(chose, bound, torch.zeros_like(bound))
    if "scores" in out:
        col = torch.arange(1, L).unsqueeze(0)
        mask = (col >= P) & (col < lengths.unsqueeze(1))
        own = torch.where(mask, out["token_logprobs"].cpu().double(), torch.zeros((), dtype=torch.float64)).sum(1)
        assert out["scores"].dtype == torch.float64 and torch.allclose(out["scores"].cpu(), own, rtol=0, atol=1e-12)
        assert bool(((out["scores"].cpu() - total).abs() <= total_bound).all())
    return total


@pytest.mark.parametrize("kind,dtype", CASES)
def test_filters_off_is_todays_call_bit_for_bit_with_no_new_cache_entry(kind, dtype):
    c = case(kind, dtype)
    eng = c["eng"]
    with torch.no_grad():
        base = eng.generate(c["lat"], L, c["prompt"], temperature=1.0, seed=5)
        entries = dict(eng._gen_cache)
        graphs = {k: g["graph"] for k, g in entries.items()}
        off = eng.generate(c["lat"], L, c["prompt"], temperature=1.0, seed=5, top_k=0, top_p=1.0, want_scores=False)
        greedy = eng.generate(c["lat"], L, c["prompt"], top_k=0, top_p=1.0)
    assert dict(eng._gen_cache) == entries and all(eng._gen_cache[k]["graph"] is g for k, g in graphs.items())
    assert set(off) == set(base) == {"ids", "lengths", "finished"}
    for k in base:
        assert torch.equal(off[k], base[k]), k
    assert torch.equal(greedy["ids"], c["greedy"]["ids"])


@pytest.mark.parametrize("kind,dtype", CASES)
def test_top_k_one_is_greedy_at_any_temperature(kind, dtype):
    c = case(kind, dtype)
    with torch.no_grad():
        for tau in (1.0, 0.5):
            out = c["eng"].generate(c["lat"], L, c["prompt"], temperature=tau, seed=7, top_k=1)
            assert torch.equal(out["ids"], c["greedy"]["ids"]) and bool((out["kept"] == 1).all()) and out["kept"].shape == (B, L - 1)
            assert "token_logprobs" not in out and "scores" not in out


@pytest.mark.parametrize("kind,dtype", CASES)
@pytest.mark.parametrize("tau,k,p", [(1.0, 50, 1.0), (0.8, 0, 0.9), (1.3, 20, 0.5)])
def test_every_free_token_lies_in_the_band_and_the_scores_match_the_reference(kind, dtype, tau, k, p):
    c = case(kind, dtype)
    with torch.no_grad():
        out = c["eng"].generate(c["lat"], L, c["prompt"], temperature=tau, seed=21, top_k=k, top_p=p, want_logits=True, want_scores=True)
    assert out["kept"].shape == out["token_logprobs"].shape == (B, L - 1) and out["scores"].shape == (B,)
    assert out["token_logprobs"].dtype == torch.float32 and out["kept"].dtype == torch.int64
    judge(out, tau, k, p)
    assert bool((out["kept"] >= 1).all()) and (k == 0 or bool((out["kept"] <= k).all()))
    assert bool((out["scores"] <= 0).all()) and bool(out["scores"].isfinite().all())


@pytest.mark.parametrize("kind,dtype", CASES)
def test_scores_count_only_the_positions_that_chose_a_token(kind, dtype):
    c = case(kind, dtype)
    eng = c["eng"]
    prompt2 = torch.cat([c["prompt"], torch.full((B, 1), 1500, dtype=torch.int64, device="cuda")], dim=1)
    with torch.no_grad():
        two = eng.generate(c["lat"], L, prompt2, temperature=1.0, seed=3, top_k=10, want_logits=True, want_scores=True)
        assert torch.equal(two["ids"][:, :2], prompt2)
        judge(two, 1.0, 10, 1.0, P=2)
        free = eng.generate(c["lat"], L, c["prompt"], temperature=1.0, seed=3, top_p=0.8, want_scores=True)
        eos = int(free["ids"][0, 3])                                            # a token this draw is seen to emit
        out = eng.generate(c["lat"], L, c["prompt"], temperature=1.0, seed=3, top_p=0.8, eos_id=eos, pad_id=7, want_logits=True, want_scores=True)
    assert bool(out["finished"][0]) and int(out["lengths"][0]) <= 4 and bool((out["ids"][0, int(out["lengths"][0]):] == 7).all())
    judge(out, 1.0, 0, 0.8)
    n = int(out["lengths"][0])
    assert abs(float(out["scores"][0]) - float(out["token_logprobs"][0, :n - 1].double().sum())) <= 1e-12
    assert torch.equal(out["ids"][0, :n], free["ids"][0, :n]) and float(out["scores"][0]) >= float(free["scores"][0])
    # the score of the greedy sentence under the full softmax
    with torch.no_grad():
        g = eng.generate(c["lat"], L, c["prompt"], want_logits=True, want_scores=True)
    assert torch.equal(g["ids"], c["greedy"]["ids"]) and bool((g["kept"] == V).all())
    total = judge(g, 0.0, 0, 1.0)
    lsm = torch.log_softmax(g["logits"].double(), dim=-1).gather(2, g["ids"][:, 1:].unsqueeze(-1)).squeeze(-1).sum(1).cpu()
    assert torch.allclose(total, lsm, rtol=0, atol=1e-9)


@pytest.mark.parametrize("kind,dtype", CASES)
def test_graph_and_eager_agree_and_one_graph_serves_every_filter_temperature_and_seed(kind, dtype):
    c = case(kind, dtype)
    eng = c["eng"]
    kw = dict(temperature=0.9, seed=13, top_k=40, top_p=0.95, want_scores=True)
    with torch.no_grad():
        a = eng.generate(c["lat"], L, c["prompt"], **kw)
        entry = next(g for k, g in eng._gen_cache.items() if "filtered" in k and g["B"] == B and g["step_logits"] is None)
        graph, replays = entry["graph"], entry["replays"]
        assert graph is not None and entry["filter"].numel() == 4
        n_entries = len(eng._gen_cache)
        eager = eng.generate(c["lat"], L, c["prompt"], graph=False, **kw)
        assert entry["replays"] == replays
        outs = [eng.generate(c["lat"], L, c["prompt"], temperature=tau, seed=seed, top_k=k, top_p=p, want_scores=True)
                for tau, seed, k, p in ((0.9, 13, 40, 0.95), (0.5, 14, 5, 1.0), (1.5, (1 << 40) + 1, 0, 0.7))]
    assert entry["graph"] is graph and entry["replays"] == replays + 3 * (L - 1) and len(eng._gen_cache) == n_entries
    for k in ("ids", "lengths", "finished", "kept", "token_logprobs", "scores"):
        assert torch.equal(a[k], eager[k]), k
        assert torch.equal(a[k], outs[0][k]), k
    assert not torch.equal(outs[1]["ids"], a["ids"]) and not torch.equal(outs[2]["ids"], a["ids"])
    assert bool((outs[1]["kept"] <= 5).all()) and bool((outs[0]["kept"] <= 40).all())
    census = eng.gen_census()
    assert len(census) >= 2
    for n in census:
        assert n["kernel"] > 0 and n["memset"] == 0 and n["memcpy"] == 0 and n["empty"] == 0 and n["event"] == 0 and n["other"] == 0, n


@pytest.mark.parametrize("dtype", [torch.bfloat16])
def test_pad_rows_never_show_and_do_not_reach_the_live_rows(dtype):
    """B = 5 (three pad rows) against the same five sentences inside B = 8 (no pad row): the noise of a row depends on its index only"""
    c = case("shelgon", dtype)
    eng = c["eng"]
    lat8 = latents_of("shelgon", c["model"], 5, n=8)[0].to(dtype).cuda().contiguous()
    prompt8 = torch.full((8, 1), START, dtype=torch.int64, device="cuda")
    kw = dict(temperature=1.0, seed=2, top_k=30, top_p=0.9, want_scores=True, want_logits=True)
    with torch.no_grad():
        small = eng.generate(lat8[:5].contiguous(), L, prompt8[:5].contiguous(), **kw)
        big = eng.generate(lat8, L, prompt8, **kw)
    assert small["ids"].shape == (5, L) and small["kept"].shape == (5, L - 1) and small["token_logprobs"].shape == (5, L - 1) and small["scores"].shape == (5,)
    for k in ("ids", "logits", "lengths", "finished", "kept", "token_logprobs", "scores"):
        assert torch.equal(small[k], big[k][:5]), k


def test_refusals_happen_before_any_launch_and_an_ordinary_call_follows():
    from kvq._ffi import KvqError
    c = case("shelgon", torch.bfloat16)
    eng, lat, prompt, idx = c["eng"], c["lat"], c["prompt"], c["idx"]
    entries = dict(eng._gen_cache)
    for kw, text in ((dict(top_k=-1, temperature=1.0), "top_k"), (dict(top_k=2.5, temperature=1.0), "top_k"), (dict(top_k=True, temperature=1.0), "top_k"),
                     (dict(top_p=0.0, temperature=1.0), "top_p"), (dict(top_p=1.2, temperature=1.0), "top_p"), (dict(top_p=float("nan"), temperature=1.0), "top_p"),
                     (dict(top_k=5), "temperature 0"), (dict(top_p=0.5, temperature=0.0), "temperature 0"),
                     (dict(top_k=5, temperature=-1.0), "temperature"), (dict(top_k=5, temperature=1.0, seed=-1), "seed")):
        with pytest.raises(KvqError, match=text):
            eng.generate(lat, L, prompt, **kw)
        with pytest.raises(KvqError, match=text):
            eng.generate_codes(idx, L, prompt, **kw)
    e = torch.randint(1000, 2000, (B, SE), generator=torch.Generator().manual_seed(11)).cuda()
    with pytest.raises(KvqError, match="free_running"):
        eng.traverse_codes(e, torch.ones_like(e), 2, 3, top_k=5, temperature=1.0)
    with pytest.raises(KvqError, match="top_k"):
        eng.traverse_codes(e, torch.ones_like(e), 2, 3, free_running=True, num_beams=2, top_k=5, temperature=1.0)
    for kw in (dict(top_k=5), dict(top_p=0.9), dict(temperature=1.0), dict(seed=1), dict(want_scores=True)):
        key = next(iter(kw))
        with pytest.raises(KvqError, match=key):
            eng.beam_search(lat, L, prompt, 2, **kw)
        with pytest.raises(KvqError, match=key):
            eng.beam_search_codes(idx, L, prompt, 2, **kw)
        with pytest.raises(KvqError, match=key):
            c["model"].generate_from_codes(idx, L, prompt, num_beams=2, **kw)
    bagon = case("bagon", torch.float32)
    with pytest.raises(KvqError, match="top_p"):
        bagon["model"].generate_from_latents(bagon["lat"], L, bagon["prompt"], num_beams=2, top_p=0.5)
    old = eng.V
    eng.V = 40000                                                                   # a vocabulary above the kernel's capacity: refused by name
    try:
        with pytest.raises(KvqError, match="vocabulary"):
            eng.generate(lat, L, prompt, temperature=1.0, top_k=5)
    finally:
        eng.V = old
    assert dict(eng._gen_cache) == entries
    with torch.no_grad():
        assert torch.equal(eng.generate(lat, L, prompt)["ids"], c["greedy"]["ids"])
        assert torch.equal(eng.beam_search(lat, L, prompt, 1)["ids"], c["greedy"]["ids"])


def test_generate_codes_traversal_and_the_model_methods_pass_the_filters_through():
    c = case("shelgon", torch.bfloat16)
    eng, idx = c["eng"], c["idx"]
    kw = dict(temperature=0.8, seed=6, top_k=12, top_p=0.9)
    with torch.no_grad():
        want = eng.generate(c["lat"], L, c["prompt"], want_scores=True, **kw)
        a = eng.generate_codes(idx, L, c["prompt"], want_scores=True, **kw)
        for k in ("ids", "lengths", "finished", "kept", "token_logprobs", "scores"):
            assert torch.equal(a[k], want[k]), k
        m = c["model"].generate_from_codes(idx, L, c["prompt"], want_scores=True, **kw)
        assert torch.equal(m["ids"], want["ids"]) and torch.equal(m["scores"], want["scores"])
        e = torch.randint(1000, 2000, (B, SE), generator=torch.Generator().manual_seed(11)).cuda()
        em = torch.ones_like(e)
        tr = eng.traverse_codes(e, em, 2, 3, free_running=True, max_length=L, start_id=START, want_scores=True, **kw)
        own = eng.encode(e, em)["indices"].reshape(B, SE, 1)[2]
        rows = own.unsqueeze(0).repeat(K, 1, 1)
        rows[:, 3, 0] = torch.arange(K, device="cuda")
        ref = eng.generate_codes(rows, L, torch.full((K, 1), START, dtype=torch.int64, device="cuda"), want_scores=True, **kw)
        assert tr["recon_ids"].shape == (K, L) and torch.equal(tr["recon_ids"], ref["ids"]) and torch.equal(tr["scores"], ref["scores"])
        mt = c["model"].traverse_codes(e, em, 2, 3, free_running=True, max_length=L, start_id=START, **kw)
        assert torch.equal(mt["recon_ids"], ref["ids"]) and "scores" not in mt
        plain = eng.traverse_codes(e, em, 2, 3, free_running=True, max_length=L, start_id=START)       # the default stays greedy
        assert torch.equal(plain["recon_ids"], eng.generate_codes(rows, L, torch.full((K, 1), START, dtype=torch.int64, device="cuda"))["ids"])
    bagon = case("bagon", torch.float32)
    with torch.no_grad():
        x = bagon["eng"].generate(bagon["lat"], L, bagon["prompt"], **kw)
        assert torch.equal(bagon["model"].generate_from_latents(bagon["lat"], L, bagon["prompt"], **kw)["ids"], x["ids"])


def _run_analysis(script, tmp_path, args=(), **overrides):
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kindergarten-vq-vae_amd")
    env = dict(os.environ)
    env.update({"PYTHONPATH": pkg, "KVQ_SYNTHETIC_SENTENCES": "200", "KVQ_BATCH_SIZE": "50",
                "KVQ_ENCODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_DECODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_VQ_E_DIM": "128",
                "KVQ_SENTENCES_PATH": repr(str(tmp_path / "data" / "dSentences_sentences.npy")),
                "KVQ_LATENT_CLASSES_LABELS_PATH": repr(str(tmp_path / "data" / "dSentences_latent_classes_labels.npy")),
                "KVQ_RUN_DIR": repr(str(tmp_path / "run"))})
    env.update(overrides)
    return subprocess.run([sys.executable, os.path.join(pkg, "analyses", *script), *args], env=env, cwd=str(tmp_path), capture_output=True,
                          text=True, timeout=600)


def test_code_traversal_script_takes_the_sampling_switches(tmp_path):
    from analyses.get_max_acc_sentences import read_table
    r = _run_analysis(("latent_traversals", "code_traversal.py"), tmp_path, args=("--free-running", "--samples", "2", "--top-k", "5", "--top-p", "0.9"),
                      KVQ_POSITIONS="[2]", KVQ_VQ_N_E="9")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    df = read_table(str(tmp_path / "run" / "code_traversal.feather"))
    assert len(df) == 9
    for col in ("sample_0", "sample_0_score", "sample_1", "sample_1_score"):
        assert col in df.columns, list(df.columns)
    assert "sample_2" not in df.columns and bool((df["sample_0_score"] <= 0).all()) and bool((df["sample_1_score"] <= 0).all())
    assert bool((df["sample_0"] != df["sample_1"]).any())                          # another seed, another draw
    # samples are drawn, not searched: refused together with beams, before any model is built
    r = _run_analysis(("latent_traversals", "code_traversal.py"), tmp_path, args=("--free-running", "--samples", "2", "--num-beams", "2"),
                      KVQ_POSITIONS="[2]", KVQ_VQ_N_E="9")
    assert r.returncode != 0 and "--num-beams" in r.stderr + r.stdout


def test_latent_arithmetics_script_takes_the_sampling_switches(tmp_path):
    from analyses.get_max_acc_sentences import read_table
    r = _run_analysis(("latent_arithmetics", "latent_arithmetics.py"), tmp_path, args=("--free-running", "--samples", "2", "--top-k", "5", "--top-p", "0.9"),
                      KVQ_MODEL_NAME="'Bagon'", KVQ_N_SENTENCES="20")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    df = read_table(str(tmp_path / "run" / "latent_arithmetics.feather"))
    assert len(df) == 20 and list(df.columns)[:3] == ["input_sentence", "recon_sentence", "edited_sentence"]
    for col in ("sample_0", "sample_0_score", "sample_1", "sample_1_score", "edited_sample_0", "edited_sample_1_score"):
        assert col in df.columns, list(df.columns)
    assert bool((df["sample_0_score"] <= 0).all())
    r = _run_analysis(("latent_arithmetics", "latent_arithmetics.py"), tmp_path, args=("--free-running", "--samples", "2"),
                      KVQ_MODEL_NAME="'Bagon'", KVQ_N_SENTENCES="20", KVQ_NUM_BEAMS="2")
    assert r.returncode != 0 and "--num-beams" in r.stderr + r.stdout
