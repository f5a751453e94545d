"""TrainEngine(loss_ignore_pad=True): reconstruction loss, accuracy and per-sentence accuracy over the tokens whose target is not
the pad id, against the f64 reference step of tests/_dropout_ref.py with
target = ids.masked_fill(ids == pad, -100) -- F.cross_entropy's default ignore_index makes that exactly the masked mean.

Models, batches and the per-tensor error are those of tests/test_engine_dropout_gpu.py; dropout is off everywhere here (the
-nodrop configurations, or training=False), so the reference needs no masks.  Every batch holds both pads and real tokens in
every sentence but the first."""
import pytest
import torch

import _ce_ignore_ref as RI
import _dropout_ref as R
from test_engine_dropout_gpu import (F32_ATOL, F32_RTOL, _bagon, _batch, _f32_exact, _perturbed, _shelgon, engine_grads, engine_weights,
                                     rel_errors)

pytestmark = pytest.mark.gpu

TINY = "kvq-bert-tiny-nodrop"


@pytest.fixture(autouse=True)
def _no_environment_switch(monkeypatch):
    for name in ("KVQ_LOSS_IGNORE_PAD", "KVQ_GRAD_ACCUM", "KVQ_MAX_GRAD_NORM", "KVQ_VQ_REVIVE_AFTER", "KVQ_WEIGHT_EMA", "KVQ_DP_SINGLE_RANK",
                 "KVQ_OWN_LMCE"):
        monkeypatch.delenv(name, raising=False)


def _padded_batch(B, S, seed, **kw):
    """_batch with at most S - 1 real tokens per sentence: pads and real tokens in every sentence (asserted for all but the first)."""
    ids, mask = _batch(B, S, seed, max_len=kw.pop("max_len", S - 1), **kw)
    real = ids[1:] != 0
    assert bool(real.any(dim=1).all()) and bool((~real).any(dim=1).all()), "a sentence without a pad or without a real token"
    return ids, mask


def _reference(eng, ids, mask, out, dec=None, target=None, masked=True):
    """The f64 step on the engine's weights and code indices; masked: pads of the target become -100 (ignored by F.cross_entropy)."""
    cfg = eng.dcfg
    tgt = target if target is not None else (dec[0] if dec is not None else ids)
    if masked:
        tgt = tgt.masked_fill(tgt == eng.pad_idx, -100)
    return R.ref_step(engine_weights(eng), ids, mask, eng.nh, eps=cfg.layer_norm_eps, dec_ids=dec[0] if dec else None,
                      dec_mask=dec[1] if dec else None, target=tgt, idx=out["indices"] if eng.has_vq else None,
                      beta=eng.beta_vq if eng.has_vq else 0.25, keep=None, p_hid=0.0, p_attn=0.0, pad_idx=eng.pad_idx)


def _from_reference_logits(ref, target, pad):
    """What the step must report, from the reference's f64 logits: (acc f32, acc_per_sentence [B] f32, count, recon_ids)."""
    target = target.cpu()
    pred = ref["logits"].argmax(dim=-1).cpu()
    real = target != pad
    count = int(real.sum())
    hits = int(((pred == target) & real).sum())
    acc = torch.tensor(hits / count, dtype=torch.float64).float()
    return acc, RI.seq_acc_ignore_ref(pred, target, pad), count, torch.where(real, pred, torch.full_like(pred, pad))


def _check_reported(out, ref, target, pad, what):
    acc, per_sentence, count, recon = _from_reference_logits(ref, target, pad)
    assert float(out["loss_tokens"]) == count and 0 < count < target.numel(), (what, float(out["loss_tokens"]), count)
    assert float(out["acc"]) == float(acc), (what, float(out["acc"]), float(acc))
    assert torch.equal(out["recon_ids"].cpu(), recon), f"{what}: recon_ids (the pad id at ignored places)"
    if out["acc_per_sentence"] is not None:
        assert torch.equal(out["acc_per_sentence"].cpu(), per_sentence), (what, out["acc_per_sentence"].cpu().tolist(), per_sentence.tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# f32, tiny: per element
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["shelgon", "bagon"])
def test_f32_tiny_step_matches_the_masked_reference(kind):
    """Every trainable tensor per element at the f32 engine test's tolerances, loss_recon to 1e-5, accuracy / per-sentence accuracy /
    token count exactly those of the reference logits; the UNMASKED reference misses the same tolerances on the same batch."""
    from kvq.engine import TrainEngine
    model = _shelgon(TINY, torch.float32) if kind == "shelgon" else _bagon(TINY, torch.float32)
    eng = TrainEngine(model, lr=1e-3, loss_ignore_pad=True)
    assert eng.loss_ignore_pad is True and eng.pad_idx == 0
    ids, mask = _padded_batch(6, 12, seed=1)
    dec = target = None
    kw = {}
    if kind == "bagon":
        dec = _perturbed(ids, mask, 0.3, 2, 1000, 2000)
        target = ids                                                  # the clean sentence, pads included
        assert bool((target == 0).any()) and not torch.equal(dec[0], target)
        kw = dict(dec_ids=dec[0], dec_mask=dec[1], target_ids=target)
    out = eng.forward_backward(ids, mask, training=True, compute_grads=True, **kw)
    torch.cuda.synchronize()
    scored = target if target is not None else ids
    ref = _reference(eng, ids, mask, out, dec, target)
    _f32_exact(eng, out, ref, f"{kind} masked")
    _check_reported(out, ref, scored, eng.pad_idx, kind)
    assert (out["acc_per_sentence"] is not None) == (kind == "bagon")
    # the control: the mean over all B * S rows is another loss and another gradient
    ref_all = _reference(eng, ids, mask, out, dec, target, masked=False)
    assert abs(float(out["loss_recon"]) - float(ref_all["loss_recon"])) > 1e-5 * abs(float(ref_all["loss_recon"]))
    grads = engine_grads(eng)
    missed = 0
    for n, g in grads.items():
        if n.endswith(".k.b"):
            continue
        try:
            torch.testing.assert_close(g, ref_all["grads"][n].float(), rtol=F32_RTOL, atol=F32_ATOL)
        except AssertionError:
            missed += 1
    assert missed > len(grads) // 2, f"only {missed} of {len(grads)} tensors tell the masked step from the unmasked reference"


def test_eval_step_and_forward_logits_score_real_tokens():
    from kvq.engine import TrainEngine
    eng = TrainEngine(_shelgon(TINY, torch.float32), lr=3e-3, loss_ignore_pad=True)
    ids, mask = _padded_batch(6, 12, seed=4)
    for _ in range(80):                                               # memorise the batch: the accuracies below are not all 0
        eng.train_step(ids, mask)
    out = eng.eval_step(ids, mask)
    print(f"after 80 steps: real-token accuracy {float(out['acc']):.3f}, per sentence {RI.seq_acc_ignore_ref(out['recon_ids'], ids, 0).tolist()}")
    assert 0 < float(out["acc"])
    ref = _reference(eng, ids, mask, out)
    assert abs(float(out["loss_recon"]) - float(ref["loss_recon"])) <= 1e-5 * abs(float(ref["loss_recon"]))
    _check_reported(out, ref, ids, eng.pad_idx, "eval_step")
    fl = eng.forward_logits(ids, mask)
    assert float(fl["loss_tokens"]) == float(out["loss_tokens"]) and float(fl["acc"]) == float(out["acc"])
    assert torch.equal(fl["recon_ids"], out["recon_ids"])


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16, bert-base widths
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bf16_bert_base_widths_error_against_the_option_off():
    """kvq-bert-base-2l Shelgon, bf16, 64 x 32 = 2048 rows, 4-12 real tokens per sentence (the corpus' range), dropout off.  e_on: worst
    per-tensor relative L2 of the option-on engine against the masked reference; e_off: the same figure of an option-off engine (the
    parent's code path) against the unmasked reference, in the same run.  Required: e_on <= 3 e_off -- 3 is the project's margin for
    bf16 bounds, and fewer contributing rows may raise the relative rounding noise by up to about sqrt(N / count) ~ 2.
    Measured on an MI355X: e_on 1.274e-2, e_off 1.273e-2 (both dec.1.sa.q.w), ratio 1.00; loss_recon error 5.7e-6 (on) and
    1.7e-6 (off); 568 of 2048 tokens counted."""
    from kvq.engine import TrainEngine
    ids, mask = _padded_batch(64, 32, seed=21, lo=1000, hi=30000, min_len=4, max_len=12)
    res = {}
    for on in (True, False):
        model = _shelgon("kvq-bert-base-2l", torch.bfloat16, K=512)
        eng = TrainEngine(model, lr=1e-4, loss_ignore_pad=on)
        out = eng.forward_backward(ids, mask, training=False, compute_grads=True)
        torch.cuda.synchronize()
        ref = _reference(eng, ids, mask, out, masked=on)
        errs = rel_errors(eng, ref)
        assert len(errs) > 60
        worst = max(errs.items(), key=lambda t: t[1])
        e_loss = abs(float(out["loss_recon"]) - float(ref["loss_recon"])) / abs(float(ref["loss_recon"]))
        res[on] = worst[1]
        print(f"loss_ignore_pad={on}: worst per-tensor relative L2 {worst[1]:.3e} ({worst[0]}), loss_recon error {e_loss:.2e}"
              + (f", {int(out['loss_tokens'])} of {ids.numel()} tokens counted" if on else ""))
        assert e_loss < 5e-5                                           # the bf16 loss tolerance of tests/test_engine_dropout_gpu.py
        if on:
            _check_count = int((ids != 0).sum())
            assert float(out["loss_tokens"]) == _check_count
        del eng, model, ref, out
        torch.cuda.empty_cache()
    e_on, e_off = res[True], res[False]
    print(f"e_on {e_on:.3e}, e_off {e_off:.3e}, ratio {e_on / e_off:.2f}")
    assert e_on <= 3 * e_off, (e_on, e_off)


def test_statistics_path_of_the_lm_head_scores_real_tokens(monkeypatch):
    """KVQ_OWN_LMCE=1 (the LM-head GEMM leaves per-tile softmax statistics, kvq_ce_forward_stats_ignore reads them): at 2048 bf16 rows
    the path is taken with the pad id, and what the forward reports is judged against f64 from the logits IT returned, at the kernel
    tests' bounds: recon_ids the first arg-max (the pad id at pads), the count exact, the accuracy within 1e-6 relative, the mean loss
    within 1e-6 + 2e-6 |ref|.  (The backward of this path is the default path's kernel.)"""
    from kvq import nnops
    from kvq.engine import TrainEngine
    ids, mask = _padded_batch(64, 32, seed=22, lo=1000, hi=30000, min_len=4, max_len=12)
    calls = []
    real = nnops.ce_forward_stats
    monkeypatch.setattr(nnops, "ce_forward_stats", lambda *a, **kw: calls.append(kw.get("ignore_index")) or real(*a, **kw))
    monkeypatch.setenv("KVQ_OWN_LMCE", "1")
    eng = TrainEngine(_shelgon("kvq-bert-base-2l", torch.bfloat16, K=512), lr=1e-4, loss_ignore_pad=True)
    out = eng.forward_logits(ids, mask)
    torch.cuda.synchronize()
    assert calls == [0], calls                                        # taken once, with the pad id
    ref = RI.ce_ignore_ref(out["logits"].reshape(ids.numel(), -1).float(), ids.reshape(-1), 0)
    assert float(out["loss_tokens"]) == ref["count"] == int((ids != 0).sum())
    assert torch.equal(out["recon_ids"].reshape(-1).cpu(), ref["pred"])
    print(f"statistics path: loss {float(out['loss_recon'])!r} against {ref['loss']!r}, acc {float(out['acc'])!r} against {ref['acc']!r}")
    assert abs(float(out["acc"]) - ref["acc"]) <= 1e-6 * ref["acc"]
    assert abs(float(out["loss_recon"]) - ref["loss"]) <= 1e-6 + 2e-6 * abs(ref["loss"])
    out = eng.forward_backward(ids, mask, training=False, compute_grads=True)      # and a training step on this path stays finite
    torch.cuda.synchronize()
    assert calls == [0, 0] and all(bool(torch.isfinite(g).all()) for g in engine_grads(eng).values())


# ---------------------------------------------------------------------------------------------------------------------------------
# the captured step
# ---------------------------------------------------------------------------------------------------------------------------------
def _run_steps(kind, monkeypatch, graph, on, steps=5):
    from kvq.engine import TrainEngine
    monkeypatch.setenv("KVQ_GRAPH", "1" if graph else "0")
    model = _shelgon(TINY, torch.float32) if kind == "shelgon" else _bagon(TINY, torch.float32)
    eng = TrainEngine(model, lr=1e-3, loss_ignore_pad=on)
    assert eng.use_graph is graph
    outs = []
    for k in range(steps):
        ids, mask = _padded_batch(8, 12, seed=30 + k)
        kw = {}
        if kind == "bagon":
            d = _perturbed(ids, mask, 0.3, 40 + k, 1000, 2000)
            kw = dict(dec_ids=d[0], dec_mask=d[1], target_ids=ids)
        o = eng.train_step(ids, mask, **kw)
        outs.append({k2: v.clone() for k2, v in o.items() if torch.is_tensor(v)})
    torch.cuda.synchronize()
    return eng, outs


@pytest.mark.parametrize("kind", ["shelgon", "bagon"])
def test_replayed_steps_equal_eager_ones_and_the_graph_keeps_its_nodes(kind, monkeypatch):
    """Five train_steps (two eager warm-ups, the capture, two replays) against five eager ones: bit-equal master weights and
    outputs.  The captured chain has the node census of an option-off engine on the same model -- the kernels are swapped one for one
    -- and holds no memset or memcpy node."""
    eng_g, outs_g = _run_steps(kind, monkeypatch, True, True)
    assert eng_g._graphs, "the step was not captured"
    eng_e, outs_e = _run_steps(kind, monkeypatch, False, True)
    assert not eng_e._graphs
    bits = lambda t: t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    assert torch.equal(bits(eng_g.flat.master), bits(eng_e.flat.master)), "master weights differ between replay and eager"
    if eng_g.has_vq:
        assert torch.equal(bits(eng_g.E.data), bits(eng_e.E.data))
    for k, (a, b) in enumerate(zip(outs_g, outs_e)):
        assert set(a) == set(b) and "loss_tokens" in a
        for name in a:
            assert torch.equal(bits(a[name]), bits(b[name])), f"step {k}: {name} differs between replay and eager"
    assert float(outs_g[-1]["loss_tokens"]) == float((_padded_batch(8, 12, seed=34)[0] != 0).sum())
    census_on = next(iter(eng_g._graphs.values())).node_census()
    eng_off, outs_off = _run_steps(kind, monkeypatch, True, False)
    assert "loss_tokens" not in outs_off[-1]
    census_off = next(iter(eng_off._graphs.values())).node_census()
    print(kind, "census on", census_on, "off", census_off)
    assert census_on == census_off
    for c in census_on:
        assert c["memset"] == 0 and c["memcpy"] == 0 and c["other"] == 0, census_on


def test_a_batch_whose_targets_are_all_pad():
    """Bagon (every gradient belongs to the reconstruction path): loss_recon = loss_tokens = 0, every gradient 0, and the optimiser
    step behind it leaves nothing non-finite -- torch would have returned NaN for this batch."""
    from kvq.engine import TrainEngine
    eng = TrainEngine(_bagon(TINY, torch.float32), lr=1e-3, loss_ignore_pad=True)
    eng.use_graph = False
    ids, mask = _padded_batch(6, 12, seed=5)
    target = torch.zeros_like(ids)
    w0 = eng.flat.master.clone()
    out = eng.train_step(ids, mask, target_ids=target)
    torch.cuda.synchronize()
    assert float(out["loss_recon"]) == 0.0 and float(out["loss_tokens"]) == 0.0 and float(out["acc"]) == 0.0
    assert not bool(out["acc_per_sentence"].any()) and bool((out["recon_ids"] == 0).all())
    for a, b in eng.flat.ranges:
        assert not bool(eng.flat.grad[a:b].any()), "a gradient of the reconstruction path is not 0"
    fl = eng.flat
    for t in (fl.master, fl.m, fl.v, fl.shadow):
        assert bool(torch.isfinite(t.float()).all())
    assert torch.equal(fl.master, w0)                                     # Adam on a zero gradient from zero moments moves nothing
    out = eng.train_step(ids, mask)                                       # and the engine goes on: a step with real tokens
    assert float(out["loss_tokens"]) == float((ids != 0).sum()) and float(out["loss_recon"]) > 0 and not torch.equal(fl.master, w0)


def test_grad_accum_normalises_each_micro_batch_by_its_own_count():
    """grad_accum = 2, f32 tiny Shelgon: the gradient Adam reads is (g1 + g2) / 2 of two masked reference steps on the weights the
    cycle began with -- (loss_i / A).backward() with ignore_index, each micro-batch divided by ITS count (the two differ)."""
    from kvq.engine import TrainEngine
    eng = TrainEngine(_shelgon(TINY, torch.float32), lr=1e-3, loss_ignore_pad=True, grad_accum=2)
    eng.use_graph = False
    W0 = {n: w.clone() for n, w in engine_weights(eng).items()}
    batches = [_padded_batch(6, 12, seed=7), _padded_batch(6, 12, seed=8, max_len=6)]
    counts, refs = [], []
    for k, (ids, mask) in enumerate(batches):
        out = eng.train_step(ids, mask)
        assert out["optimizer_step"] is (k == 1)
        counts.append(float(out["loss_tokens"]))
        cfg = eng.dcfg
        refs.append(R.ref_step(W0, ids, mask, eng.nh, eps=cfg.layer_norm_eps, target=ids.masked_fill(ids == 0, -100), idx=out["indices"],
                               beta=eng.beta_vq, pad_idx=0))
    assert counts[0] != counts[1] and counts == [float((b[0] != 0).sum()) for b in batches]
    got = {}
    for n, p in eng.param_of.items():
        if p.requires_grad:
            o, cnt, shape = eng.flat.seg[n]
            got[n] = eng.flat.acc[o:o + cnt].view(shape)
    got["vq.E"] = [a for a in eng.aux if a["p"].requires_grad][0]["acc"].view(eng.E.shape)
    assert len(got) > 60
    for n, g in got.items():
        want = ((refs[0]["grads"][n] + refs[1]["grads"][n]) / 2).float()
        if n.endswith(".k.b"):
            q = n[:-3] + "q.b"
            assert g.norm().item() <= F32_RTOL * ((refs[0]["grads"][q] + refs[1]["grads"][q]) / 2).norm().item(), n
            continue
        torch.testing.assert_close(g.float(), want.view(g.shape), rtol=F32_RTOL, atol=F32_ATOL, msg=lambda m: f"{n}: {m}")


# ---------------------------------------------------------------------------------------------------------------------------------
# decode(), the training state, the autograd path
# ---------------------------------------------------------------------------------------------------------------------------------
def test_decode_scores_real_tokens():
    from kvq.engine import TrainEngine
    model = _shelgon(TINY, torch.float32).eval()
    eng = TrainEngine(model, lr=1e-3, loss_ignore_pad=True)
    ids, mask = _padded_batch(6, 12, seed=9)
    lat = eng.encode(ids, mask)
    res = eng.decode(lat["z_q"].contiguous(), ids, mask, want_logits=True)
    pred = res["logits"].argmax(dim=-1).cpu()
    t = ids.cpu()
    real = t != 0
    assert torch.equal(res["acc_per_sentence"].cpu(), RI.seq_acc_ignore_ref(pred, t, 0))
    assert torch.equal(res["recon_ids"].cpu(), torch.where(real, pred, torch.zeros_like(pred)))
    assert float(res["loss_tokens"]) == int(real.sum())
    assert float(res["acc"]) == float(torch.tensor(int(((pred == t) & real).sum()) / int(real.sum()), dtype=torch.float64).float())
    off = TrainEngine(_shelgon(TINY, torch.float32).eval(), lr=1e-3).decode(lat["z_q"].contiguous(), ids, mask)
    assert "loss_tokens" not in off and torch.equal(off["recon_ids"].cpu()[real], res["recon_ids"].cpu()[real])
    assert bool((off["recon_ids"].cpu()[~real] != 0).any()), "the option-off engine reports the arg-max at pads as well"


def test_training_state_carries_the_option():
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    on = TrainEngine(_shelgon(TINY, torch.float32), lr=1e-3, loss_ignore_pad=True)
    off = TrainEngine(_shelgon(TINY, torch.float32), lr=1e-3)
    assert on.state_fingerprint()["loss_ignore_pad"] is True and "loss_ignore_pad" not in off.state_fingerprint()
    assert set(on.state_fingerprint()) - set(off.state_fingerprint()) == {"loss_ignore_pad"}
    ids, mask = _padded_batch(6, 12, seed=10)
    on.train_step(ids, mask)
    off.train_step(ids, mask)
    with pytest.raises(KvqError, match="fingerprint.loss_ignore_pad"):
        off.load_state_dict(on.state_dict())
    with pytest.raises(KvqError, match="fingerprint.loss_ignore_pad"):
        on.load_state_dict(off.state_dict())
    again = TrainEngine(_shelgon(TINY, torch.float32), lr=1e-3, loss_ignore_pad=True)
    again.load_state_dict(on.state_dict())
    assert torch.equal(again.flat.master, on.flat.master)


def test_a_model_without_a_pad_id_is_refused():
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    model = _bagon(TINY, torch.float32)
    model.encoder.embeddings.word_embeddings.padding_idx = None
    model.decoder.bert.embeddings.word_embeddings.padding_idx = None
    with pytest.raises(KvqError, match="padding_idx"):
        TrainEngine(model, lr=1e-3, loss_ignore_pad=True)
    assert TrainEngine(model, lr=1e-3).loss_ignore_pad is False


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("inplace", [False, True])
def test_fused_cross_entropy_with_ignore_index(dtype, inplace):
    """N = 37, V = 1027, pad id 0, against the f64 reference at the kernel tests' bounds (tests/_pointwise_ref.py)."""
    import _pointwise_ref as P
    from kvq.functional import fused_cross_entropy
    N, V, pad, g_loss = 37, 1027, 0, 1.7
    g = torch.Generator().manual_seed(50)
    x = (2 * torch.randn(N, V, generator=g)).to(dtype)
    t = torch.randint(1, V, (N,), generator=g)
    t[torch.rand(N, generator=g) < 0.6] = pad
    assert 0 < int((t != pad).sum()) < N
    ref = RI.ce_ignore_ref(x.float(), t, pad, g_loss)
    logits = x.cuda().requires_grad_(True)
    work = logits * 1                                                 # a non-leaf the in-place backward may overwrite
    loss, acc, pred = fused_cross_entropy(work.view(1, N, V), t.cuda().view(1, N), inplace_backward=inplace, ignore_index=pad)
    (loss * g_loss).backward()
    assert pred.shape == (1, N) and torch.equal(pred.cpu().view(-1), ref["pred"])
    assert abs(float(loss.detach()) - ref["loss"]) <= 1e-6 + 2e-6 * abs(ref["loss"]) and abs(float(acc) - ref["acc"]) <= 1e-6 * ref["acc"]
    grad = logits.grad.cpu()
    assert not bool(grad[t == pad].any())
    safe_t = torch.where(t == pad, torch.zeros_like(t), t)
    r = P.ce_grad_ratio(grad, ref, dtype == torch.bfloat16, safe_t)
    assert float(r.max()) <= 1, float(r.max())
    # and without ignore_index nothing changed: the mean over all rows
    l0, a0, p0 = fused_cross_entropy(x.cuda(), t.cuda())
    assert abs(float(l0) - float(P.ce_ref(x.float(), t)["row_loss"].mean())) <= 1e-6 + 2e-6 * abs(float(l0))
