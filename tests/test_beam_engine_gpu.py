"""TrainEngine.beam_search / beam_search_codes and the num_beams switch of the wrappers: the beam search over the key/value cache
against generate() (one beam), against the f64 reference of tests/_beam_ref.py on its own trace, and against the teacher-forced
decode() of the same engine (causality).

Models, latents and prompts: the cases of tests/test_generate_engine_gpu.py (kvq-bert-tiny Shelgon and Bagon, V = 2048, H = 128;
B = 6, Se = 12, L = 20, P = 1, seed SEED), W = 4; a second case B = 3, W = 3, P = 4, whose R = 9 rows are padded to 16.

Every step is judged on the kernel's own inputs: the trace's logits of the step and its previous step_scores (BR.judge_choices: the
tolerance and the "decided" rule derived in tests/_beam_ref.py); at most 5 % of the (sentence, step) pairs may be undecided -- a
condition of the test (profiles/beam_search.md has the share of the HF f32 modules alone on the CPU, and the run's).
Causality: decode(latents[b], beam_ids[b, w]) teacher-forced gives at position j - 1 the logits token j was scored with; each
log-probability moves by at most the chosen logit's and the log-sum-exp's error, each at most tol, over n generated tokens:
|beam_scores - sum_j log softmax| <= n * 2 tol, tol = 2 (2e-4 + 2e-4 max |x|) in f32 and 3 E_TF in bf16 (the figures of
tests/test_generate_engine_gpu.py).
"""
import functools

import numpy as np
import pytest
import torch

import _beam_ref as BR
from test_generate_engine_gpu import ATOL, B, CASES, E_TF_MEASURED, K, L, RTOL, SE, START, V, _run_analysis, case, latents_of

pytestmark = pytest.mark.gpu

W = 4
# latents of the searches, chosen on the CPU with the HF f32 modules alone (logits rounded to bf16 for the bf16 engine): the seeds with
# the fewest undecided (sentence, step) pairs of a search over several hundred; shares in profiles/beam_search.md
BEAM_SEED = {"shelgon": 71, "bagon": 307}
PAD_SEED = 97                            # the B = 3, W = 3, P = 4 case (prompts: seed 6, as tests/test_generate_engine_gpu.py)


@functools.lru_cache(maxsize=None)
def beams(kind, dtype):
    """the engine of the generate tests' case on this file's own latents (BEAM_SEED), generate() and beam_search() on them"""
    c = dict(case(kind, dtype))
    eng = c["eng"]
    lat32, idx = latents_of(kind, c["model"], BEAM_SEED[kind])
    c.update(lat=lat32.to(dtype).cuda().contiguous(), idx=None if idx is None else idx.cuda())
    fixed = tuple(t.cuda() for t in (torch.randint(1000, 2000, (B, SE), generator=torch.Generator().manual_seed(9)), torch.ones(B, SE, dtype=torch.int64)))
    with torch.no_grad():
        c["gen"] = eng.generate(c["lat"], L, c["prompt"], want_logits=True)
        c["G"] = c["gen"]["ids"]
        gen_before = eng.generate(c["lat"], L, c["prompt"], want_logits=True)
        fwd_before = eng.forward_logits(*fixed)["logits"].clone()
        out = eng.beam_search(c["lat"], L, c["prompt"], W, want_trace=True)
        fwd_after = eng.forward_logits(*fixed)["logits"].clone()
        gen_after = eng.generate(c["lat"], L, c["prompt"], want_logits=True)
    torch.cuda.synchronize()
    return dict(c, out=out, gen_before=gen_before, gen_after=gen_after, fwd_before=fwd_before, fwd_after=fwd_after)


def replay_trace(trace, n, Wn, P, prompt, eos, pad):
    """Every step of a search redone in f64 from the trace -> (the final host state, decided pairs, all pairs, worst score error /
    tolerance).  The bookkeeping the trace does not carry (finished, lengths, ancestry) follows from the kernel's own choices."""
    ids, parent, ss = (trace[k].cpu().numpy().reshape(n * Wn, -1) for k in ("ids", "parent", "step_scores"))
    logits = trace["logits"].cpu().numpy().reshape(n * Wn, ids.shape[1] - 1, -1)
    Lh = ids.shape[1]
    st = BR.new_state(n, Wn, Lh, prompt.cpu().numpy(), pad, R=n * Wn)
    probe = dict(ids=ids, parent=parent, step_scores=ss)
    decided_n = pairs = 0
    worst = 0.0
    for t in range(Lh - 1):
        replay = None
        if t + 1 >= P:
            decided, w, replay = BR.judge_choices(st, BR.choices_of(probe, Wn, t), logits[:, t], logits.shape[2], Wn, t, eos, pad)
            decided_n, pairs, worst = decided_n + sum(decided), pairs + len(decided), max(worst, w)
        st = BR.book(st, replay, Wn, t, P, eos, pad)
        for k in probe:                                                # the trace is the bookkeeping of the kernel's own choices
            assert np.array_equal(st[k][:, t + 1], probe[k][:, t + 1]), (k, t)
    return st, decided_n, pairs, worst


@functools.lru_cache(maxsize=None)
def main_steps(kind, dtype):
    c = beams(kind, dtype)
    return check_against_trace(c["out"], B, W, 1, c["prompt"])


def check_against_trace(out, n, Wn, P, prompt, eos=None, pad=0, alpha_zero=True):
    st, decided, pairs, worst = replay_trace(out["trace"], n, Wn, P, prompt, eos, pad)
    Lh = st["ids"].shape[1]
    hyp = BR.gather_ref(st, Lh - 1, pad).reshape(n, Wn, Lh)
    for r in range(n * Wn):                                            # hypotheses = the backtrack of the trace through `parent`
        m = int(st["lengths"][r])
        assert np.array_equal(hyp.reshape(n * Wn, Lh)[r, :m], BR.backtrack(st["ids"], st["parent"], r, Lh - 1)[:m]), r
    if alpha_zero:                                                     # the final order is the slot order
        assert np.array_equal(out["beam_ids"].cpu().numpy(), hyp)
        assert np.array_equal(out["beam_scores"].cpu().numpy(), st["scores"].reshape(n, Wn))
        assert np.array_equal(out["beam_lengths"].cpu().numpy(), st["lengths"].reshape(n, Wn))
        assert np.array_equal(out["beam_finished"].cpu().numpy(), st["finished"].reshape(n, Wn) != 0)
    return st, hyp, decided, pairs, worst


@pytest.mark.parametrize("kind,dtype", CASES)
def test_one_beam_is_generate_bit_for_bit(kind, dtype):
    c = beams(kind, dtype)
    with torch.no_grad():
        one = c["eng"].beam_search(c["lat"], L, c["prompt"], 1, want_trace=True)
    gen = c["gen"]
    for k in ("ids", "lengths", "finished"):
        assert torch.equal(one[k], gen[k]), k
    assert one["beam_ids"].shape == (B, 1, L) and torch.equal(one["beam_ids"][:, 0], gen["ids"])
    assert torch.equal(one["trace"]["logits"][:, 0], gen["logits"])     # the same step, the same bits
    # its score is the sum of the log-softmax of its own step logits at the chosen tokens (f64); the steps' tolerances add up
    x = one["trace"]["logits"][:, 0].double()
    lse = torch.logsumexp(x, dim=-1)
    lp = x.gather(-1, gen["ids"][:, 1:].unsqueeze(-1)).squeeze(-1) - lse
    err = (one["beam_scores"][:, 0].double() - lp.sum(1)).abs()
    tol = (BR.TOL_ABS + BR.TOL_REL * (lse.abs() + lp.abs() + lp.cumsum(1).abs())).sum(1)
    assert bool((err <= tol).all()), (err.max().item(), tol.min().item())
    check_against_trace(one, B, 1, 1, c["prompt"])


@pytest.mark.parametrize("kind,dtype", CASES)
def test_every_step_is_the_top_w_of_its_own_logits(kind, dtype):
    c = beams(kind, dtype)
    out = c["out"]
    assert out["beam_ids"].shape == (B, W, L) and out["beam_scores"].shape == (B, W) and out["beam_scores"].dtype == torch.float32
    assert out["trace"]["logits"].shape == (B, W, L - 1, V) and out["ids"].shape == (B, L) and out["lengths"].shape == (B,)
    st, hyp, decided, pairs, worst = main_steps(kind, dtype)
    print(f"\n[beam_search steps {kind} {dtype}] {pairs - decided} of {pairs} (sentence, step) pairs undecided; worst score error / tolerance = {worst:.3f}")
    assert pairs == B * (L - 1) and decided > 0.8 * pairs               # (the 5 % condition: test_at_most_five_percent_... below)
    assert torch.equal(out["ids"], out["beam_ids"][:, 0]) and torch.equal(out["lengths"], out["beam_lengths"][:, 0])
    assert bool((out["beam_ids"][:, :, 0] == START).all()) and bool((out["beam_scores"][:, :-1] >= out["beam_scores"][:, 1:]).all())
    assert all(len({tuple(h) for h in hyp[b].tolist()}) == W for b in range(B))      # W different sentences


@pytest.mark.parametrize("kind,dtype", CASES)
def test_scores_are_the_teacher_forced_log_probabilities_of_the_hypotheses(kind, dtype):
    c = beams(kind, dtype)
    out, eng = c["out"], c["eng"]
    hyp = out["beam_ids"].reshape(B * W, L)
    with torch.no_grad():
        tf = eng.decode(c["lat"].repeat_interleave(W, dim=0).contiguous(), hyp, torch.ones_like(hyp), want_logits=True)["logits"].double()
    lp = torch.log_softmax(tf[:, :L - 1], dim=-1).gather(-1, hyp[:, 1:].unsqueeze(-1)).squeeze(-1)           # [B W, L - 1]: token j from row j - 1
    n = L - 1                                                           # (no end token: every hypothesis has L - 1 generated tokens)
    assert bool((out["beam_lengths"] == L).all())
    if dtype == torch.float32:
        tol = 2 * (ATOL + RTOL * tf[:, :L - 1].abs().amax(-1))          # per position
    else:
        tol = torch.full_like(lp, 3 * E_TF_MEASURED[kind])
    err = (out["beam_scores"].reshape(-1).double() - lp.sum(1)).abs()
    bound = (2 * tol).sum(1)
    print(f"\n[beam_search causality {kind} {dtype}] max |score - teacher-forced sum| = {err.max().item():.3e} over n = {n} tokens; "
          f"worst error / bound = {(err / bound).max().item():.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("kind,dtype", CASES)
def test_graph_and_eager_agree_and_nothing_else_moves(kind, dtype):
    c = beams(kind, dtype)
    eng, out = c["eng"], c["out"]
    entry = next(g for g in eng._beam_cache.values() if g["B"] == B and g["W"] == W and g["step_logits"] is not None)
    graph, replays = entry["graph"], entry["replays"]
    assert graph is not None and replays >= L - 1
    with torch.no_grad():
        eager = eng.beam_search(c["lat"], L, c["prompt"], W, want_trace=True, graph=False)
        assert entry["replays"] == replays
        again = eng.beam_search(c["lat"], L, c["prompt"], W, want_trace=True)
    assert entry["graph"] is graph and entry["replays"] == replays + L - 1          # the second call replays the first call's graph
    for other in (eager, again):
        for k in ("ids", "lengths", "finished", "beam_ids", "beam_scores", "beam_lengths", "beam_finished"):
            assert torch.equal(other[k], out[k]), k
        for k in ("ids", "parent", "step_scores", "logits"):
            assert torch.equal(other["trace"][k], out["trace"][k]), k
    census = eng.gen_census()
    assert len(census) >= 2
    for n in census:
        assert n["kernel"] > 0 and n["memset"] == 0 and n["memcpy"] == 0 and n["empty"] == 0 and n["event"] == 0 and n["other"] == 0, n
    for k in ("ids", "logits", "lengths", "finished"):                 # generate() around a beam call: the same bits
        assert torch.equal(c["gen_before"][k], c["gen"][k]) and torch.equal(c["gen_after"][k], c["gen"][k]), k
    assert torch.equal(c["fwd_before"], c["fwd_after"])


@functools.lru_cache(maxsize=None)
def eos_steps(dtype):
    c = beams("shelgon", dtype)
    eng, ref = c["eng"], c["out"]
    eos, pad = int(ref["beam_ids"][0, 0, 3]), 7                          # a token the reference run's best hypothesis emits
    with torch.no_grad():
        out = eng.beam_search(c["lat"], L, c["prompt"], W, eos_id=eos, pad_id=pad, want_trace=True)
        pen = eng.beam_search(c["lat"], L, c["prompt"], W, eos_id=eos, pad_id=pad, length_penalty=1.0)
    return (out, pen, eos, pad) + check_against_trace(out, B, W, 1, c["prompt"], eos=eos, pad=pad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_end_token_finished_hypotheses_compete_and_length_penalty_reranks(dtype):
    out, pen, eos, pad, st, hyp, decided, pairs, _ = eos_steps(dtype)
    assert pairs == B * (L - 1) and decided > 0.8 * pairs
    fin, lens, ids = out["beam_finished"], out["beam_lengths"], out["beam_ids"]
    assert bool(fin.any())
    for b in range(B):
        for w in range(W):
            n = int(lens[b, w])
            if bool(fin[b, w]):
                assert int(ids[b, w, n - 1]) == eos and bool((ids[b, w, n:] == pad).all()) and not bool((ids[b, w, 1:n - 1] == eos).any())
            else:
                assert n == L and not bool((ids[b, w, 1:] == eos).any())
    # a finished hypothesis kept the score of the step that finished it, through every slot it lived in afterwards
    ss, anc = out["trace"]["step_scores"].cpu().numpy().reshape(B * W, L), st["anc"][(L - 1) & 1]
    for r in np.nonzero(st["finished"][:B * W])[0]:
        for j in range(int(st["lengths"][r]) - 1, L):
            assert ss[anc[r, j], j] == st["scores"][r], (r, j)
    # length_penalty = 1: the host's key order, the same hypotheses and raw scores
    key = out["beam_scores"].double() / (lens - 1).clamp(min=1).double()
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    assert torch.equal(pen["beam_scores"], out["beam_scores"].gather(1, order))
    assert torch.equal(pen["beam_ids"], ids.gather(1, order.unsqueeze(-1).expand(B, W, L)))
    assert torch.equal(pen["ids"], pen["beam_ids"][:, 0]) and torch.equal(pen["finished"], fin.gather(1, order)[:, 0])
    assert "trace" not in pen


@functools.lru_cache(maxsize=None)
def pad_steps(dtype):
    c = case("shelgon", dtype)
    eng = c["eng"]
    lat8 = latents_of("shelgon", c["model"], PAD_SEED, n=8)[0].to(dtype).cuda().contiguous()
    prompt8 = torch.randint(1000, 2000, (8, 4), generator=torch.Generator().manual_seed(6)).cuda()
    prompt8[:, 0] = START
    lat3, prompt3 = lat8[:3].contiguous(), prompt8[:3].contiguous()
    with torch.no_grad():
        small = eng.beam_search(lat3, L, prompt3, 3, want_trace=True)
        big = eng.beam_search(lat8[:5].contiguous(), L, prompt8[:5].contiguous(), 3, want_trace=True)
        entry = next(g for g in eng._beam_cache.values() if g["B"] == 3 and g["W"] == 3)
        assert entry["R"] == 16 and entry["S"] == 6
        entry["lat"][3:].fill_(float("nan"))                            # the pad sentences' latents: poisoned
        poisoned = eng.beam_search(lat3, L, prompt3, 3, want_trace=True)
        entry["lat"][3:].zero_()
    return (small, big, poisoned, prompt3) + check_against_trace(small, 3, 3, 4, prompt3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pad_rows_never_show_and_do_not_reach_the_live_rows(dtype):
    """B = 3, W = 3, P = 4: R = 9 rows padded to 16, a last sentence of one row; against the same sentences inside B = 5 (R = 15
    padded to 16 as well: the same launches, two more live sentences where the first run has pad rows)"""
    small, big, poisoned, prompt3, _, _, decided, pairs, _ = pad_steps(dtype)
    assert small["beam_ids"].shape == (3, 3, L) and small["trace"]["logits"].shape == (3, 3, L - 1, V) and small["ids"].shape == (3, L)
    assert bool((small["beam_ids"][:, :, :4] == prompt3.unsqueeze(1)).all())      # the prompt is kept
    for k in ("ids", "beam_ids", "beam_scores", "beam_lengths", "beam_finished"):
        assert torch.equal(small[k], big[k][:3]), k
        assert torch.equal(small[k], poisoned[k]), k
    for k in ("ids", "parent", "step_scores", "logits"):
        assert torch.equal(small["trace"][k], poisoned["trace"][k]), k
    assert torch.equal(small["trace"]["logits"], big["trace"]["logits"][:3])
    assert bool(torch.isfinite(small["beam_scores"]).all())
    assert pairs == 3 * (L - 4) and decided > 0.8 * pairs


def test_at_most_five_percent_of_the_step_pairs_are_undecided():
    """The condition of every token-for-token comparison in this file, over all (sentence, step) pairs it judges: the four searches
    of B = 6, W = 4, the two with an end token, the two of B = 3, W = 3.  bf16 logits carry 8 significant bits, so two of a beam's
    best five tokens tie outright in 9 % (Shelgon) to 16 % (Bagon) of the pairs of a typical seed -- the seeds are the best of a
    search on the CPU with the HF f32 modules alone (profiles/beam_search.md), and the share is taken over the file, not per case."""
    runs = [main_steps(kind, dtype)[2:4] for kind, dtype in CASES] + [eos_steps(d)[6:8] for d in (torch.float32, torch.bfloat16)] \
        + [pad_steps(d)[6:8] for d in (torch.float32, torch.bfloat16)]
    decided, pairs = sum(r[0] for r in runs), sum(r[1] for r in runs)
    print(f"\n[beam_search] undecided (sentence, step) pairs per run: {[r[1] - r[0] for r in runs]} of {[r[1] for r in runs]}; "
          f"together {pairs - decided} of {pairs} = {(pairs - decided) / pairs:.4f}")
    assert pairs - decided <= 0.05 * pairs


def test_refusals_happen_before_any_launch_and_an_ordinary_call_follows():
    from kvq._ffi import KvqError
    c = beams("shelgon", torch.float32)
    eng, lat, prompt = c["eng"], c["lat"], c["prompt"]
    calls = {"beam_search": lambda: eng.beam_search(lat, L, prompt, W), "beam_search_codes": lambda: eng.beam_search_codes(c["idx"], L, prompt, W)}
    for attr, value, text in (("_cap", object(), "graph capture"), ("group", object(), "process group"), ("fp8", True, "fp8")):
        old = getattr(eng, attr)
        setattr(eng, attr, value)
        try:
            for fn in calls.values():
                with pytest.raises(KvqError, match=text):
                    fn()
        finally:
            setattr(eng, attr, old)
    for nb in (0, 9, -1, True, 2.0, None, V + 1):
        with pytest.raises(KvqError, match="num_beams"):
            eng.beam_search(lat, L, prompt, nb)
        with pytest.raises(KvqError, match="num_beams"):
            eng.beam_search_codes(c["idx"], L, prompt, nb)
    for lp in (float("inf"), float("nan"), "1", None, True):
        with pytest.raises(KvqError, match="length_penalty"):
            eng.beam_search(lat, L, prompt, W, length_penalty=lp)
        with pytest.raises(KvqError, match="length_penalty"):
            eng.beam_search_codes(c["idx"], L, prompt, W, length_penalty=lp)
    with pytest.raises(KvqError, match="sequence length"):              # everything generate refuses
        eng.beam_search(lat, 40, prompt, W)
    with pytest.raises(KvqError, match="position table"):
        eng.beam_search(lat, 65, prompt, W)
    with pytest.raises(KvqError, match="latents must be"):
        eng.beam_search(lat[:, :, :64].contiguous(), L, prompt, W)
    with pytest.raises(KvqError, match="contiguous"):
        eng.beam_search(lat.bfloat16(), L, prompt, W)
    with pytest.raises(KvqError, match="prompt_ids must be"):
        eng.beam_search(lat, L, prompt[:4], W)
    with pytest.raises(KvqError, match="does not fit"):
        eng.beam_search(lat, 3, torch.full((B, 4), START, dtype=torch.int64, device="cuda"), W)
    for kw, text in ((dict(eos_id=V), "eos_id"), (dict(pad_id=-1), "pad_id")):
        with pytest.raises(KvqError, match=text):
            eng.beam_search(lat, L, prompt, W, **kw)
        with pytest.raises(KvqError, match=text):
            eng.beam_search_codes(c["idx"], L, prompt, W, **kw)
    with pytest.raises(TypeError):
        eng.beam_search(lat, L, prompt, W, temperature=1.0)             # sampled beams are out of scope: no such argument
    bad_prompt = prompt.clone()
    bad_prompt[3, 0] = V
    with pytest.raises(KvqError, match="prompt_ids hold ids outside"):
        eng.beam_search(lat, L, bad_prompt, W)
    with pytest.raises(KvqError, match="no quantiser"):
        case("bagon", torch.float32)["eng"].beam_search(case("bagon", torch.float32)["lat"], L, prompt, W, quantize=True)
    with pytest.raises(KvqError, match="quantize"):
        eng.beam_search_codes(c["idx"], L, prompt, W, quantize=True)
    with torch.no_grad():
        q = eng.beam_search(lat, L, prompt, W, quantize=True)           # codebook rows quantise to themselves
        assert torch.equal(q["indices"].reshape(B, SE), c["idx"]) and torch.equal(q["beam_ids"], c["out"]["beam_ids"])
        assert torch.equal(eng.beam_search(lat, L, prompt, W)["beam_scores"], c["out"]["beam_scores"])


def test_wrappers_route_to_beam_search_and_one_beam_is_todays_call():
    for dtype in (torch.float32, torch.bfloat16):
        c = beams("shelgon", dtype)
        eng, model, idx, out = c["eng"], c["model"], c["idx"], c["out"]
        with torch.no_grad():
            a = eng.beam_search_codes(idx, L, c["prompt"], W)
            assert torch.equal(a["beam_ids"], out["beam_ids"]) and torch.equal(a["beam_scores"], out["beam_scores"]) and "trace" not in a
            m = model.generate_from_codes(idx, L, c["prompt"], num_beams=W)
            assert torch.equal(m["beam_ids"], out["beam_ids"]) and torch.equal(m["ids"], out["ids"])
            assert torch.equal(model.generate_from_codes(idx, L, c["prompt"], num_beams=1)["ids"], c["G"]) and "beam_ids" not in \
                model.generate_from_codes(idx, L, c["prompt"])
            e = torch.randint(1000, 2000, (B, SE), generator=torch.Generator().manual_seed(11)).cuda()
            em = torch.ones_like(e)
            tr = model.traverse_codes(e, em, 2, 3, free_running=True, max_length=L, start_id=START, num_beams=2)
            own = eng.encode(e, em)["indices"].reshape(B, SE, 1)[2]
            rows = own.unsqueeze(0).repeat(K, 1, 1)
            rows[:, 3, 0] = torch.arange(K, device="cuda")
            want = eng.beam_search_codes(rows, L, torch.full((K, 1), START, dtype=torch.int64, device="cuda"), 2)
            one = model.traverse_codes(e, em, 2, 3, free_running=True, max_length=L, start_id=START, num_beams=1)
            greedy = eng.traverse_codes(e, em, 2, 3, free_running=True, max_length=L, start_id=START)
        assert tr["recon_ids"].shape == (K, L) and torch.equal(tr["recon_ids"], want["ids"])
        assert torch.equal(tr["beam_ids"], want["beam_ids"]) and torch.equal(tr["beam_scores"], want["beam_scores"])
        assert torch.equal(tr["changed"], want["ids"] != want["ids"][tr["own_code"]].unsqueeze(0))
        assert torch.equal(one["recon_ids"], greedy["recon_ids"]) and "beam_ids" not in one
    b = beams("bagon", torch.bfloat16)
    with torch.no_grad():
        m = b["model"].generate_from_latents(b["lat"], L, b["prompt"], num_beams=W, length_penalty=0.0)
        assert torch.equal(m["beam_ids"], b["out"]["beam_ids"]) and torch.equal(m["beam_scores"], b["out"]["beam_scores"])
        assert torch.equal(b["model"].generate_from_latents(b["lat"], L, b["prompt"], num_beams=1)["ids"], b["G"])


def test_code_traversal_script_takes_the_num_beams_switch(tmp_path):
    """the command-line form; the table gains the score and runner-up columns"""
    from analyses.get_max_acc_sentences import read_table
    out = _run_analysis(("latent_traversals", "code_traversal.py"), tmp_path, args=("--free-running", "--num-beams", "2"), KVQ_POSITIONS="[2]",
                        KVQ_VQ_N_E="9")
    assert "variants" in out
    df = read_table(str(tmp_path / "run" / "code_traversal.feather"))
    assert len(df) == 9 and sorted(set(df["code"])) == list(range(9))
    assert {"score", "runner_up_1", "runner_up_1_score"} <= set(df.columns) and "runner_up_2" not in df.columns
    assert bool((df["score"] >= df["runner_up_1_score"]).all())


def test_latent_arithmetics_script_takes_the_num_beams_constant(tmp_path):
    """the configuration form (KVQ_NUM_BEAMS)"""
    from analyses.get_max_acc_sentences import read_table
    out = _run_analysis(("latent_arithmetics", "latent_arithmetics.py"), tmp_path, KVQ_MODEL_NAME="'Bagon'", KVQ_N_SENTENCES="20",
                        KVQ_FREE_RUNNING="True", KVQ_NUM_BEAMS="3")
    assert "edited" in out
    df = read_table(str(tmp_path / "run" / "latent_arithmetics.feather"))
    assert list(df.columns)[:3] == ["input_sentence", "recon_sentence", "edited_sentence"] and len(df) == 20
    for side in ("recon_", "edited_"):
        assert {side + "score", side + "runner_up_1", side + "runner_up_2_score"} <= set(df.columns)
        assert bool((df[side + "score"] >= df[side + "runner_up_1_score"]).all())
