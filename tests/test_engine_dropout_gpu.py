"""The TrainEngine's dropout-ON step against an f64 reference under the same masks (tests/_dropout_ref.py).

Every other gradient-parity test of the engine runs with dropout off.  Here a forward_backward(training=True) runs, then every mask
the step used is recovered from the kernels' own entry points at the engine's (step seed, site) -- kvq_dropout for the embedding
dropout, kvq_dropout_residual_ln_fwd on ones for a hidden dropout, kvq_attn_fwd with q = k = 0 and one-hot V rows for the attention
probabilities -- with the site of each block read from what the engine's own block functions return.  The f64 reference then
runs with those masks, the engine's code indices and the engine's weights (bf16 shadow; LayerNorm parameters from the f32
master the kernels read), and losses plus EVERY trainable parameter tensor (the codebook included) are compared per tensor by
relative L2.  A backward that regenerated a mask from another site or another seed offset would fail this; replay-equals-eager,
fused-equals-unfused and falling-loss checks would not.

key.bias: its true gradient is zero (softmax is shift invariant along the keys), so its norm is bounded relative to the norm of
the query.bias gradient of the same block instead.

Bounds (worst per-tensor relative L2 over all trainable tensors; bf16 bounds fixed at <= 3x the largest error measured on an
MI355X, measurements in each test's docstring).
"""
import pytest
import torch

import _dropout_ref as R

pytestmark = pytest.mark.gpu

F32_RTOL, F32_ATOL = 2e-3, 2e-6               # the dropout-off f32 test (tests/test_engine_gpu.py), per element
BOUND = {                                      # bf16, per tensor relative L2 (see the docstrings for what was measured)
    "base_8192": 3e-2,
    "bagon_base": 3e-2,
    "base_s64": 3e-2,
}
LOSS_RTOL = {"f32": 1e-5, "bf16": 5e-5}        # measured: <= 6.7e-8 (f32), <= 1.9e-5 (bf16)


# ---------------------------------------------------------------------------------------------------------------------------------
# models and batches
# ---------------------------------------------------------------------------------------------------------------------------------
def _shelgon(name, dtype, K=32, seed=0):
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(seed)
    H = 128 if "tiny" in name else 768
    vq = VectorQuantizer(K, H, 0.25, vq_codebook_init_values=torch.randn(K, H))
    vq.materialize_min_encodings = False
    model = Shelgon(name, vq, name, None, compute_dtype=dtype).cuda()
    model.set_mode("full")
    return model.train()


def _bagon(name, dtype, seed=0):
    from models.bagon.Bagon import Bagon
    torch.manual_seed(seed)
    model = Bagon(name, name, True, compute_dtype=dtype).cuda()
    model.set_mode("full")
    return model.train()


def _batch(B, S, seed, lo=1000, hi=2000, min_len=3, max_len=None):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(lo, hi, (B, S), generator=g)
    lens = torch.randint(min_len, (max_len or S) + 1, (B,), generator=g)
    lens[0] = max_len or S
    ids = ids * (torch.arange(S)[None] < lens[:, None])
    return ids.cuda(), (ids != 0).long().cuda()


def _perturbed(ids, mask, pct, seed, lo, hi):
    """The decoder's own ids (models/bagon/Trainer.py:85-94): a share of the real tokens replaced by random ones."""
    g = torch.Generator().manual_seed(seed)
    swap = (torch.rand(ids.shape, generator=g) < pct).cuda() & mask.bool()
    d = torch.where(swap, torch.randint(lo, hi, ids.shape, generator=g).cuda(), ids)
    assert not torch.equal(d, ids)
    return d, mask.clone()


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine's step, its masks, the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def engine_step(eng, ids, mask, dec=None, training=True):
    """forward_backward(compute_grads=True) with the (key, kind, p, site, geometry) of every dropout recorded from what the
    engine's block functions return."""
    sites = []
    real_emb, real_attn, real_ffn = eng._emb_fwd, eng._attn_block_fwd, eng._ffn_fwd

    def emb(prefix, cfg, t, tr, **kw):
        out, saved = real_emb(prefix, cfg, t, tr, **kw)
        if saved[4] is not None:
            sites.append((prefix[:-1], "emb", saved[4][0], saved[4][1], tuple(out.shape)))
        return out, saved

    def attn(pre, *a, **kw):
        out, saved = real_attn(pre, *a, **kw)
        causal, p_attn, p_hid, site_a, site_o, B, Sq, Sk = saved[9:17]
        if p_attn > 0:
            sites.append((pre + "attn", "attn", p_attn, site_a, (B, eng.nh, Sq, Sk, bool(causal))))
        if p_hid > 0:
            sites.append((pre + "out", "hid", p_hid, site_o, tuple(out.shape)))
        return out, saved

    def ffn(pre, *a, **kw):
        out, saved = real_ffn(pre, *a, **kw)
        if saved[-2] > 0:
            sites.append((pre + "ffn", "hid", saved[-2], saved[-1], tuple(out.shape)))
        return out, saved

    eng._emb_fwd, eng._attn_block_fwd, eng._ffn_fwd = emb, attn, ffn
    try:
        kw = dict(dec_ids=dec[0], dec_mask=dec[1]) if dec is not None else {}
        out = eng.forward_backward(ids, mask, training=training, compute_grads=True, **kw)
    finally:
        del eng._emb_fwd, eng._attn_block_fwd, eng._ffn_fwd
    torch.cuda.synchronize()
    return out, sites


def reveal_masks(eng, sites):
    """{key: keep mask (f32 0 / 1)} of every recorded dropout, drawn by the kernels' own entry points at the engine's seed."""
    from kvq import nnops
    dev, dt, H = eng.dev, eng.dtype, eng.H
    keep = {}
    nnops.set_seed_offset(eng._state)
    try:
        for key, kind, p, site, geo in sites:
            if kind == "emb":
                k = nnops.dropout(torch.ones(geo, dtype=dt, device=dev), p, eng._step_seed, site) != 0
            elif kind == "hid":
                ones = torch.ones(geo, dtype=dt, device=dev)
                _, pre, _, _ = nnops.ln_fwd(ones, None, torch.ones(H, device=dev), torch.zeros(H, device=dev), 1e-12, p,
                                            eng._step_seed, site)
                k = pre.float() > 0
            else:
                B, nh, Sq, Sk, causal = geo
                assert Sk <= 64, "one-hot V rows reveal at most 64 keys"
                q0 = torch.zeros(B * Sq, H, dtype=dt, device=dev)
                k0 = torch.zeros(B * Sk, H, dtype=dt, device=dev)
                eye = torch.zeros(Sk, 64, device=dev)
                eye[torch.arange(Sk), torch.arange(Sk)] = 1
                v1 = eye[None, :, None, :].expand(B, Sk, nh, 64).reshape(B * Sk, H).to(dt).contiguous()
                ctx, _ = nnops.attn_fwd(q0, k0, v1, None, B, nh, Sq, Sk, causal, p, eng._step_seed, site)
                k = ctx.float().reshape(B, Sq, nh, 64)[..., :Sk].permute(0, 2, 1, 3) > 0          # [B, nh, Sq, Sk]
                if causal:                                  # keys after the query carry no probability: their mask is moot
                    k = k | ~torch.ones(Sq, Sk, dtype=torch.bool, device=dev).tril()
            keep[key] = k.float()
    finally:
        nnops.set_seed_offset(None)
    torch.cuda.synchronize()
    return keep


def check_masks(sites, keep):
    """Each mask keeps 1 - p +- 0.01 of its elements (attention: of the causally visible ones; +- 4 standard deviations of the
    binomial rate where that is wider, the tiny model's masks hold ~1000 elements) and no two sites share one."""
    seen = {}
    for key, kind, p, site, geo in sites:
        k = keep[key]
        if kind == "attn" and geo[4]:
            vis = torch.ones(geo[2], geo[3], dtype=torch.bool, device=k.device).tril().expand_as(k)
            rate, n = k[vis].mean().item(), int(vis.sum().item())
        else:
            rate, n = k.mean().item(), k.numel()
        tol = max(0.01, 4 * (p * (1 - p) / n) ** 0.5)
        assert abs(rate - (1 - p)) < tol, (key, rate, tol)
        for other, ok in seen.items():
            if ok.shape == k.shape:
                assert not torch.equal(ok, k), f"{key} draws the mask of {other}"
        seen[key] = k
    assert len({s[3] for s in sites}) == len(sites), "two dropouts share a site"


def engine_weights(eng):
    """The weights the engine's kernels read: bf16 / f32 shadow, LayerNorm parameters from the f32 master, the f32 codebook."""
    W = {}
    for n in eng.param_of:
        ln = n.endswith("ln.w") or n.endswith("ln.b") or n.endswith("ln2.w") or n.endswith("ln2.b")
        W[n] = eng.flat.w32(n) if ln else eng.flat.w(n)
    if eng.has_vq:
        W["vq.E"] = eng.E.detach()
    return W


def engine_grads(eng):
    g = {n: eng.flat.g(n).float() for n, p in eng.param_of.items() if p.requires_grad}
    if eng.has_vq and eng.E.requires_grad:
        g["vq.E"] = eng.gE.float()
    return g


def reference(eng, ids, mask, out, keep, dec=None, training=True):
    cfg = eng.dcfg
    p_hid = cfg.hidden_dropout_prob if training else 0.0
    p_attn = cfg.attention_probs_dropout_prob if training else 0.0
    assert (eng.ecfg.hidden_dropout_prob, eng.ecfg.attention_probs_dropout_prob) == (cfg.hidden_dropout_prob, cfg.attention_probs_dropout_prob)
    return R.ref_step(engine_weights(eng), ids, mask, eng.nh, eps=cfg.layer_norm_eps, dec_ids=dec[0] if dec else None,
                      dec_mask=dec[1] if dec else None, idx=out["indices"] if eng.has_vq else None,
                      beta=eng.beta_vq if eng.has_vq else 0.25, keep=keep if training else None, p_hid=p_hid, p_attn=p_attn,
                      pad_idx=eng.pad_idx)


def rel_errors(eng, ref, grads=None):
    """{tensor: relative L2 error}; key.bias as |g| / |g(query.bias)| of its block."""
    grads = engine_grads(eng) if grads is None else grads
    err = {}
    for n, g in grads.items():
        r = ref["grads"][n].to(g.device)
        if n.endswith(".k.b"):
            err[n] = g.double().norm().item() / ref["grads"][n[:-3] + "q.b"].norm().item()
        else:
            err[n] = (g.double() - r).norm().item() / max(r.norm().item(), 1e-300)
    return err


def loss_errors(out, ref):
    e = {"loss_recon": abs(out["loss_recon"].item() - ref["loss_recon"].item()) / abs(ref["loss_recon"].item())}
    if ref["loss_vq"] is not None:
        e["loss_vq"] = abs(out["loss_vq"].item() - ref["loss_vq"].item()) / abs(ref["loss_vq"].item())
    return e


def run_case(eng, ids, mask, dec=None, training=True):
    """One engine step + (with dropout) its revealed masks + the reference: (out, sites, keep, ref, {tensor: error})."""
    out, sites = engine_step(eng, ids, mask, dec, training)
    keep = reveal_masks(eng, sites) if training else None
    if training:
        check_masks(sites, keep)
    ref = reference(eng, ids, mask, out, keep, dec, training)
    return out, sites, keep, ref, rel_errors(eng, ref)


def assert_within(errs, bound, what):
    worst = max(errs.items(), key=lambda t: t[1])
    print(f"{what}: worst per-tensor relative L2 {worst[1]:.3e} ({worst[0]}), bound {bound:.1e}")
    bad = {n: e for n, e in errs.items() if not e <= bound}
    assert not bad, f"{what}: {len(bad)} tensors above {bound}: {sorted(bad.items(), key=lambda t: -t[1])[:8]}"


def _n_sites(eng):
    return 1 + 3 * eng.n_enc_layers + 1 + 5 * eng.n_dec_layers


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------------
def _f32_exact(eng, out, ref, what):
    """f32 engine: every tensor per element at the dropout-off f32 test's tolerance; losses to 1e-5."""
    for k, e in loss_errors(out, ref).items():
        assert e < LOSS_RTOL["f32"], (what, k, e)
    grads = engine_grads(eng)
    assert len(grads) > 60
    for n, g in grads.items():
        r = ref["grads"][n].float()
        if n.endswith(".k.b"):
            assert g.norm().item() <= F32_RTOL * ref["grads"][n[:-3] + "q.b"].norm().item(), n
            continue
        torch.testing.assert_close(g, r, rtol=F32_RTOL, atol=F32_ATOL, msg=lambda m: f"{what} {n}: {m}")


@pytest.mark.parametrize("kind", ["shelgon", "bagon"])
def test_f32_tiny_engine_with_dropout_matches_the_reference_under_its_masks(kind):
    """kvq-bert-tiny, f32, p = 0.1 everywhere: the sharp check of the mask bookkeeping (Bagon with decoder ids != encoder ids).
    Measured worst per-tensor relative L2: Shelgon 8.6e-7 (8.8e-7 with dropout off on the same batch), Bagon 8.6e-7 (7.4e-7)."""
    from kvq.engine import TrainEngine
    model = _shelgon("kvq-bert-tiny", torch.float32) if kind == "shelgon" else _bagon("kvq-bert-tiny", torch.float32)
    eng = TrainEngine(model, lr=1e-3)
    ids, mask = _batch(6, 12, seed=1)
    dec = _perturbed(ids, mask, 0.3, 2, 1000, 2000) if kind == "bagon" else None
    out, sites, keep, ref, errs = run_case(eng, ids, mask, dec)
    assert len(sites) == _n_sites(eng)
    _f32_exact(eng, out, ref, kind)


def test_f32_tiny_engine_with_dropout_after_an_optimiser_step():
    """One train_step first (graphs on), so the device step count is 1 and every dropout seed carries a non-zero offset: the masks
    revealed at that offset are the ones forward and backward used.  Measured worst per-tensor relative L2 2.7e-6 (1.1e-6 off)."""
    from kvq import nnops
    from kvq.engine import TrainEngine
    model = _shelgon("kvq-bert-tiny", torch.float32)
    eng = TrainEngine(model, lr=1e-3)
    assert eng.use_graph
    ids, mask = _batch(6, 12, seed=3)
    eng.train_step(ids, mask)
    assert eng.step_count == 1 and nnops.read_step_state(eng._state)[0] == 1
    out, sites, keep, ref, errs = run_case(eng, ids, mask)
    _f32_exact(eng, out, ref, "after one step")


def _bf16_case(eng, ids, mask, bound, what, dec=None):
    out, sites, keep, ref, errs = run_case(eng, ids, mask, dec)
    assert len(sites) == _n_sites(eng)
    for k, e in loss_errors(out, ref).items():
        assert e < LOSS_RTOL["bf16"], (what, k, e)
    assert len(errs) > 60
    assert_within(errs, bound, what)
    return out, sites, ref, errs


@pytest.mark.parametrize("fuse", [None, "1"])
def test_bf16_bert_base_widths_at_the_benchmarked_batch(fuse, monkeypatch):
    """kvq-bert-base-2l, bf16, 256 x 32 = 8192 rows (bench.py's batch): persistent QKV, grouped 256 x 256 weight gradients, the
    batched cross-K/V projection, the padded LM head; KVQ_FUSE_DROPRES at its default (two-kernel dropout + LayerNorm) and 1
    (dropout + residual in the dense layer's epilogue, bit for bit the same step).  Measured on an MI355X, both settings: worst
    per-tensor relative L2 1.30e-2 (dec.1.sa.q.w; 1.23e-2 with dropout off on the same batch), key.bias / query.bias 1.7e-3,
    losses 6.6e-7 (recon) and 1.7e-5 (quantiser).  Bound 3e-2."""
    from kvq.engine import TrainEngine
    if fuse is None:
        monkeypatch.delenv("KVQ_FUSE_DROPRES", raising=False)
    else:
        monkeypatch.setenv("KVQ_FUSE_DROPRES", fuse)
    from dsentences.synthetic import random_token_batch
    from kvq import nnops
    model = _shelgon("kvq-bert-base-2l", torch.bfloat16, K=512)
    eng = TrainEngine(model, lr=1e-4)
    ids, mask = random_token_batch(256, 32, torch.Generator().manual_seed(11))
    fused, real = [], nnops.gemm_dropres
    monkeypatch.setattr(nnops, "gemm_dropres", lambda *a, **kw: fused.append(a[4]) or real(*a, **kw))
    _bf16_case(eng, ids.cuda(), mask.cuda(), BOUND["base_8192"], f"base 8192 rows fuse={fuse}")
    n_hid = 2 * eng.n_enc_layers + 3 * eng.n_dec_layers
    assert fused == ([] if fuse is None else [0.1] * n_hid), fused        # the epilogue ran, with dropout, at every hidden dropout


def _bagon_base():
    from dsentences.synthetic import random_token_batch
    from kvq.engine import TrainEngine
    model = _bagon("kvq-bert-base-2l", torch.bfloat16)
    eng = TrainEngine(model, lr=1e-4)
    ids, mask = random_token_batch(64, 32, torch.Generator().manual_seed(12))
    ids, mask = ids.cuda(), mask.cuda()
    return eng, ids, mask, _perturbed(ids, mask, 0.3, 13, 1000, 30000)


def test_bf16_bagon_at_bert_base_widths():
    """Bagon, kvq-bert-base-2l, bf16, 64 x 32 = 2048 rows, decoder ids perturbed (30 % of the real tokens).  Measured on an MI355X:
    worst per-tensor relative L2 1.42e-2 (dec.1.ca.q.w; 1.38e-2 with dropout off), key.bias / query.bias 2.3e-3, loss 3.9e-7.
    Bound 3e-2."""
    eng, ids, mask, dec = _bagon_base()
    _bf16_case(eng, ids, mask, BOUND["bagon_base"], "bagon base", dec)


def test_bf16_64_token_sentences_run_the_blocked_attention_dropout():
    """kvq-bert-base-2l Shelgon, bf16, 32 x 64 tokens: the blocked attention kernels (above 32 tokens) and their dropout.  Measured
    on an MI355X: worst per-tensor relative L2 1.37e-2 (dec.1.sa.q.w; 1.34e-2 with dropout off), key.bias / query.bias 6.9e-3,
    losses 8.7e-6 and 1.9e-5.  Bound 3e-2."""
    from kvq.engine import TrainEngine
    model = _shelgon("kvq-bert-base-2l", torch.bfloat16, K=512)
    eng = TrainEngine(model, lr=1e-4)
    ids, mask = _batch(32, 64, seed=14, lo=1000, hi=30000, min_len=20)
    _bf16_case(eng, ids, mask, BOUND["base_s64"], "base S=64")


# ---------------------------------------------------------------------------------------------------------------------------------
# sensitivity: the bounds above reject the bugs they exist for
# ---------------------------------------------------------------------------------------------------------------------------------
def mutate_site(monkeypatch, fn_name, site, calls):
    """nnops.<fn_name> regenerates its mask from site + 1 on the call that carries `site` (once)."""
    from kvq import nnops
    real = getattr(nnops, fn_name)
    pos = 7 if fn_name == "ln_bwd_partial" else 12             # positional index of `site`

    def wrong(*a, **kw):
        a = list(a)
        if a[pos] == site and not calls:
            calls.append(site)
            a[pos] = site + 1
        return real(*a, **kw)

    monkeypatch.setattr(nnops, fn_name, wrong)


def mutate_defer(eng, dst, calls):
    """TrainEngine._defer drops the last partial row of the reduction that writes `dst` (once)."""
    real = eng._defer

    def short(src, d, count, cols, ld, src_offset=0):
        if d.data_ptr() == dst.data_ptr() and not calls:
            assert count >= 2
            calls.append(count)
            count -= 1
        return real(src, d, count, cols, ld, src_offset=src_offset)

    eng._defer = short


MUTATION_TOUCHES = {
    "ln_bwd_partial": ["dec.0.f2.w", "dec.0.f2.b", "dec.0.f1.w", "dec.0.f1.b"],     # the mask of dec.0's FFN output dropout
    "attn_bwd": ["dec.1.ca.q.w", "dec.1.ca.q.b", "dec.1.ca.k.w", "dec.1.ca.v.w"],   # the probabilities of dec.1's cross-attention
    "defer": ["dec.1.f2.b", "dec.1.ln2.w", "dec.1.ln2.b"],                          # dec.1's FFN LayerNorm / bias partial sums
}


def run_site_mutations(monkeypatch, eng, ids, mask, dec, sites, ref):
    """{mutation: {tensor: error}}: each backward of MUTATION_TOUCHES regenerates its mask from the wrong site, on a fresh step,
    judged against the unmutated reference."""
    site_of = {s[0]: s[3] for s in sites}
    res = {}
    for name, site in (("ln_bwd_partial", site_of["dec.0.ffn"]), ("attn_bwd", site_of["dec.1.ca.attn"])):
        calls = []
        with monkeypatch.context() as m:
            mutate_site(m, name, site, calls)
            engine_step(eng, ids, mask, dec)
        assert calls == [site], (name, calls)
        res[name] = rel_errors(eng, ref)
    return res


def run_defer_mutation(eng, ids, mask, dec, ref):
    calls = []
    mutate_defer(eng, eng.flat.g("dec.1.f2.b"), calls)
    try:
        engine_step(eng, ids, mask, dec)
    finally:
        del eng._defer
    assert len(calls) == 1, calls
    return rel_errors(eng, ref), calls[0]


def test_the_bf16_bound_rejects_a_mask_regenerated_from_the_wrong_site(monkeypatch):
    """On the Bagon bert-base case and its bound: (1) the LayerNorm backward of dec.0's FFN output and (2) the attention backward of
    dec.1's cross-attention regenerate their mask from site + 1 (the next dropout's).  Each weight / bias gradient the mutated call
    feeds directly misses the bound by 3x or more.  Measured on an MI355X against the bound 3e-2: (1) f2.w 0.40, f2.b 0.39,
    f1.w 0.41, f1.b 0.40; (2) q.w 0.57, q.b 0.61, v.w 0.12 (v.b 0.080 is not asserted: 2.7x)."""
    eng, ids, mask, dec = _bagon_base()
    out, sites, keep, ref, errs = run_case(eng, ids, mask, dec)
    bound = BOUND["bagon_base"]
    assert_within(errs, bound, "bagon base, unmutated")
    res = run_site_mutations(monkeypatch, eng, ids, mask, dec, sites, ref)
    for name, r in res.items():
        got = {n: r[n] for n in MUTATION_TOUCHES[name]}
        print(name, {n: f"{e:.3e}" for n, e in got.items()})
        assert all(e >= 3 * bound for e in got.values()), (name, got, bound)


def test_the_f32_check_rejects_a_lost_partial_row():
    """The deferred reduction of dec.1's FFN LayerNorm backward (partial rows of 16 tokens: [f2.b | ln2.w | ln2.b] in one launch)
    loses its last partial row, on the f32 tiny Shelgon case (72 tokens, 5 partial rows).  The three gradients it feeds miss the
    per-element check and their relative L2 error is >= 3x its rtol.  (In bf16 at 2048 rows the same loss is 1/128 of the tokens:
    0.7 % on f2.b, the size of the bf16 step's own error on that tensor -- which is why the f32 case is the sharp one.)"""
    from kvq.engine import TrainEngine
    model = _shelgon("kvq-bert-tiny", torch.float32)
    eng = TrainEngine(model, lr=1e-3)
    ids, mask = _batch(6, 12, seed=1)
    out, sites, keep, ref, errs = run_case(eng, ids, mask)
    _f32_exact(eng, out, ref, "unmutated")
    errs, rows = run_defer_mutation(eng, ids, mask, None, ref)
    got = {n: errs[n] for n in MUTATION_TOUCHES["defer"]}
    print("defer", rows, "partial rows:", {n: f"{e:.3e}" for n, e in got.items()})
    assert all(e >= 3 * F32_RTOL for e in got.values()), got
    grads = engine_grads(eng)
    for n in MUTATION_TOUCHES["defer"]:
        with pytest.raises(AssertionError):
            torch.testing.assert_close(grads[n], ref["grads"][n].float(), rtol=F32_RTOL, atol=F32_ATOL)
