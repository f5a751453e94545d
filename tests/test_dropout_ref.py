"""CPU check of tests/_dropout_ref.py, the f64 reference the dropout-on engine step is judged by (tests/test_engine_dropout_gpu.py):
against f64 autograd through HuggingFace's own BERT modules (oracle/step_oracle.py) with the same masks written into HF's dropouts
-- the hidden / embedding ones through forward hooks on its nn.Dropout modules, the attention-probability ones through the
functional dropout of its eager attention -- and the quantiser's indices from the oracle's CPU quantiser."""
import contextlib

import pytest
import torch
from torch.nn.functional import kl_div, log_softmax, one_hot

import _dropout_ref as R

CFG = "kvq-bert-tiny"
TOL = dict(rtol=1e-10, atol=1e-12)


@contextlib.contextmanager
def _f64():
    old, threads = torch.get_default_dtype(), torch.get_num_threads()
    torch.set_default_dtype(torch.float64)          # the oracle's quantiser builds its one-hot in the default dtype
    torch.set_num_threads(min(threads, 4))
    try:
        yield
    finally:
        torch.set_default_dtype(old)
        torch.set_num_threads(threads)


def _cfg():
    from models.bagon.Bagon import LOCAL_BERT_CONFIGS
    return dict(LOCAL_BERT_CONFIGS[CFG])


def _batch(B=3, S=12, seed=1, lo=1000, hi=2000):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(lo, hi, (B, S), generator=g)
    lens = torch.randint(3, S + 1, (B,), generator=g)
    lens[0] = S
    ids = ids * (torch.arange(S)[None] < lens[:, None])
    return ids, (ids != 0).long()


@contextlib.contextmanager
def _hf_masks(model, keep, p_hid, p_attn):
    """HuggingFace's forward with the given keep masks at every dropout (the model stays in eval mode: HF's own dropouts are off)."""
    import torch.nn.functional as F
    hooks, attn_queue = [], []
    n_enc, n_dec = len(model.encoder.encoder.layer), len(model.decoder.bert.encoder.layer)

    def hook(key):
        def fn(mod, inp, out):
            k = keep.get(key)
            return out if k is None else out * (k.reshape(out.shape).to(out.dtype) / (1 - p_hid))
        return fn

    def on(mod, key):
        hooks.append(mod.register_forward_hook(hook(key)))

    on(model.encoder.embeddings.dropout, "enc.emb")
    on(model.decoder.bert.embeddings.dropout, "dec.emb")
    for side, layers in (("enc", model.encoder.encoder.layer), ("dec", model.decoder.bert.encoder.layer)):
        for i, l in enumerate(layers):
            on(l.attention.output.dropout, f"{side}.{i}.sa.out")
            on(l.output.dropout, f"{side}.{i}.ffn")
            if side == "dec":
                on(l.crossattention.output.dropout, f"{side}.{i}.ca.out")
    # attention probabilities: F.dropout on a 4-D tensor, called in forward order by the eager attention
    attn_queue[:] = [k for k, kind in R.site_keys(n_enc, n_dec) if kind == "attn"]
    real = F.dropout

    def fake(x, p=0.5, training=True, inplace=False):
        if x.dim() == 4:
            k = keep.get(attn_queue.pop(0))
            return x if k is None else x * (k.to(x.dtype) / (1 - p_attn))
        return real(x, p, training, inplace)

    for m in (model.encoder, model.decoder):
        m.set_attn_implementation("eager")
    F.dropout = fake
    try:
        yield attn_queue
    finally:
        F.dropout = real
        for h in hooks:
            h.remove()


def _oracle(kind, seed=0):
    from oracle import step_oracle as SO
    torch.manual_seed(seed)
    if kind == "shelgon":
        return SO.OracleShelgon(_cfg(), n_e=32, e_dim=128, beta=0.25, codebook_init=torch.randn(32, 128)).eval()
    return SO.OracleBagon(_cfg()).eval()


def _hf_step(model, ids, mask, dec_ids=None, dec_mask=None):
    for p in model.parameters():
        p.grad = None
    V = _cfg()["vocab_size"]
    if hasattr(model, "vector_quantizer"):
        vq_loss, _perp, idx, logits = model(ids, mask)
        target = ids
    else:
        logits = model(ids, mask, dec_ids, dec_mask)
        vq_loss, idx, target = None, None, dec_ids
    loss = kl_div(input=log_softmax(logits.reshape(-1, V), dim=-1), target=one_hot(target, V).reshape(-1, V).to(logits.dtype),
                  reduction="batchmean")                                                    # Trainer.py:94-98
    (loss + vq_loss if vq_loss is not None else loss).backward()
    return dict(loss_recon=loss.detach(), loss_vq=vq_loss.detach() if vq_loss is not None else None, logits=logits.detach(), idx=idx)


def _random_keep(B, S, Sd, H, nh, n_enc, n_dec, p, seed):
    g = torch.Generator().manual_seed(seed)
    keep = {}
    for key, kind in R.site_keys(n_enc, n_dec):
        side_len = S if key.startswith("enc") else Sd
        if kind == "attn":
            shape = (B, nh, side_len, S if ".ca." in key else side_len)
        else:
            shape = (B * side_len, H)
        keep[key] = (torch.rand(shape, generator=g) >= p).to(torch.float64)
    return keep


def _compare(model, hf, ref):
    torch.testing.assert_close(ref["loss_recon"], hf["loss_recon"], **TOL)
    if hf["loss_vq"] is not None:
        torch.testing.assert_close(ref["loss_vq"], hf["loss_vq"], **TOL)
    torch.testing.assert_close(ref["logits"], hf["logits"], **TOL)
    names = R.engine_names(model)
    for n, p in names.items():
        assert p.grad is not None, n
        torch.testing.assert_close(ref["grads"][n], p.grad, **TOL, msg=lambda m: f"{n}: {m}")
    return names


@pytest.mark.parametrize("kind", ["shelgon", "bagon"])
def test_reference_with_masks_off_equals_f64_autograd_through_huggingface(kind):
    """All masks ones, indices from the oracle's quantiser: loss, logits and every parameter gradient (the codebook included) to 1e-10."""
    with _f64():
        model = _oracle(kind)
        ids, mask = _batch()
        dec_ids, dec_mask = _batch(seed=2)
        if kind == "bagon":
            dec_ids, dec_mask = dec_ids[:, :9].contiguous(), dec_mask[:, :9].contiguous()
            assert not torch.equal(dec_ids, ids[:, :9])
        else:
            dec_ids = dec_mask = None
        hf = _hf_step(model, ids, mask, dec_ids, dec_mask)
        W = {n: p.detach() for n, p in R.engine_names(model).items()}
        cfg = _cfg()
        Sd = ids.shape[1] if dec_ids is None else dec_ids.shape[1]
        ones = {k: torch.ones_like(v) for k, v in _random_keep(3, ids.shape[1], Sd, 128, cfg["num_attention_heads"],
                                                               2, 2, 0.0, 0).items()}
        ref = R.ref_step(W, ids, mask, cfg["num_attention_heads"], dec_ids=dec_ids, dec_mask=dec_mask, idx=hf["idx"], keep=ones)
        names = _compare(model, hf, ref)
        assert ("vq.E" in names) == (kind == "shelgon") and len(names) > 60


@pytest.mark.parametrize("kind", ["shelgon", "bagon"])
def test_reference_with_random_masks_equals_huggingface_with_the_same_masks(kind):
    """p = 0.1 at every dropout, each mask drawn independently: the reference and HF's modules under the same masks agree to 1e-10,
    and the result differs from the masks-off step (the masks reach the computation)."""
    p = 0.1
    cfg = _cfg()
    nh = cfg["num_attention_heads"]
    with _f64():
        model = _oracle(kind)
        ids, mask = _batch(seed=3)
        dec_ids, dec_mask = (None, None) if kind == "shelgon" else _batch(seed=4, S=10)
        Sd = ids.shape[1] if dec_ids is None else dec_ids.shape[1]
        keep = _random_keep(3, ids.shape[1], Sd, 128, nh, 2, 2, p, 7)
        with _hf_masks(model, keep, p, p) as queue:
            hf = _hf_step(model, ids, mask, dec_ids, dec_mask)
            assert queue == []                           # every attention dropout of HF's forward was given its mask
        W = {n: q.detach() for n, q in R.engine_names(model).items()}
        ref = R.ref_step(W, ids, mask, nh, dec_ids=dec_ids, dec_mask=dec_mask, idx=hf["idx"], keep=keep, p_hid=p, p_attn=p)
        _compare(model, hf, ref)
        off = R.ref_step(W, ids, mask, nh, dec_ids=dec_ids, dec_mask=dec_mask, idx=hf["idx"])
        assert (off["loss_recon"] - ref["loss_recon"]).abs() > 1e-3


def test_one_zeroed_mask_element_changes_exactly_what_it_should():
    """One kept element dropped (p = 0, so nothing else is rescaled).  In the last decoder FFN output and in the last cross-attention's
    probabilities only that token's logits move, and the reference equals HuggingFace with the same single zero.  In the encoder's
    embedding dropout, with the code indices held, the decoder and its gradients stay where they were (z_q = E[idx] feeds it) while
    the quantiser loss and every encoder gradient move."""
    cfg = _cfg()
    nh = cfg["num_attention_heads"]
    with _f64():
        model = _oracle("shelgon")
        ids, mask = _batch(seed=5)
        B, S = ids.shape
        hf0 = _hf_step(model, ids, mask)
        W = {n: q.detach() for n, q in R.engine_names(model).items()}
        base = R.ref_step(W, ids, mask, nh, idx=hf0["idx"])
        n_tok, col = 7, 5                                # token 7 of sentence 0 (all 12 of its tokens are real)
        # (1) hidden dropout of the last decoder FFN: only token n_tok's logits change
        k = torch.ones(B * S, 128)
        k[n_tok, col] = 0
        keep = {"dec.1.ffn": k}
        with _hf_masks(model, keep, 0.0, 0.0):
            hf = _hf_step(model, ids, mask)
        ref = R.ref_step(W, ids, mask, nh, idx=hf0["idx"], keep=keep)
        _compare(model, hf, ref)
        moved = (ref["logits"] != base["logits"]).any(-1).reshape(-1)
        assert moved.nonzero().reshape(-1).tolist() == [n_tok]
        assert not torch.equal(ref["grads"]["dec.1.f2.w"], base["grads"]["dec.1.f2.w"])
        # (2) attention probability (sentence 0, head 1, query 7, key 3) of the last cross-attention
        ka = torch.ones(B, nh, S, S)
        ka[0, 1, 7, 3] = 0
        keep = {"dec.1.ca.attn": ka}
        with _hf_masks(model, keep, 0.0, 0.0):
            hf = _hf_step(model, ids, mask)
        ref = R.ref_step(W, ids, mask, nh, idx=hf0["idx"], keep=keep)
        _compare(model, hf, ref)
        moved = (ref["logits"] != base["logits"]).any(-1).reshape(-1)
        assert moved.nonzero().reshape(-1).tolist() == [7]
        # (3) the encoder's embedding dropout: through the quantiser the change reaches the loss only via the codebook
        # term and via the straight-through gradient; the indices are held fixed, so the decoder's input does not move
        ke = torch.ones(B * S, 128)
        ke[n_tok, col] = 0
        keep = {"enc.emb": ke}
        ref = R.ref_step(W, ids, mask, nh, idx=hf0["idx"], keep=keep)
        torch.testing.assert_close(ref["logits"], base["logits"], **TOL)          # (z + (z_q - z) rounds, in the last bit)
        torch.testing.assert_close(ref["loss_recon"], base["loss_recon"], **TOL)
        assert ref["loss_vq"] != base["loss_vq"]
        for n in ("dec.0.sa.q.w", "head.t.w", "dec.emb.word"):
            torch.testing.assert_close(ref["grads"][n], base["grads"][n], **TOL)
        for n in ("enc.0.sa.q.w", "enc.emb.ln.w", "vq.E"):
            assert (ref["grads"][n] - base["grads"][n]).norm() > 1e-6 * base["grads"][n].norm(), n
