"""f64 reference of one Shelgon / Bagon training step in which every dropout mask and the quantiser's code indices are given by the
caller -- the checker of the TrainEngine's dropout-on step (tests/test_engine_dropout_gpu.py).

Plain torch ops over the model's parameters, in the engine's segment names (kvq/engine.py, TrainEngine.__init__):
    embeddings (word + position + token type 0) -> LayerNorm -> dropout                    modeling_bert.py:53-108
    self-attention: key-padding mask (+ causal in the decoder), dropout on the probabilities   :139-204
    cross-attention of the decoder on the quantised encoder output, no encoder mask         :206-280 (Shelgon.py:71)
    dense -> dropout -> LayerNorm(. + residual)                                             :282-296, :339-352
    FFN: dense -> GELU (erf) -> dense                                                       :325-352
    LM head: dense -> GELU -> LayerNorm -> tied decoder word table + bias                   :466-497
    loss: mean token cross entropy over every decoder position (pads included, target = decoder input by default)
    Shelgon: VectorQuantizer.py:76-80 with z_q = E[idx] and the straight-through estimator; Bagon: no quantiser.

Masks are 0 / 1 "keep" tensors, keyed by the names site_keys() lists; a kept element is scaled by 1 / (1 - p).  A key that is
absent means no dropout at that site.  Shapes: [N, H] for the embedding and hidden dropouts, [B, nh, Sq, Sk] for the attention
probabilities (Sq = Sk = the side's length for self-attention, Sq = decoder length, Sk = encoder length for cross-attention).
"""
from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn.functional as F


def engine_names(model) -> Dict[str, torch.nn.Parameter]:
    """{engine segment name: parameter} for a model with `encoder` (BertModel), `decoder` (BertLMHeadModel) and optionally
    `vector_quantizer.embedding` (the codebook, named "vq.E") -- the names TrainEngine.param_of uses."""
    out = {}

    def emb(prefix, e):
        out[prefix + "word"] = e.word_embeddings.weight
        out[prefix + "pos"] = e.position_embeddings.weight
        out[prefix + "type"] = e.token_type_embeddings.weight
        out[prefix + "ln.w"], out[prefix + "ln.b"] = e.LayerNorm.weight, e.LayerNorm.bias

    def attn(prefix, a):
        s = a.self
        for k, lin in (("q", s.query), ("k", s.key), ("v", s.value), ("o", a.output.dense)):
            out[prefix + k + ".w"], out[prefix + k + ".b"] = lin.weight, lin.bias
        out[prefix + "ln.w"], out[prefix + "ln.b"] = a.output.LayerNorm.weight, a.output.LayerNorm.bias

    def layer(prefix, l, cross):
        attn(prefix + "sa.", l.attention)
        if cross:
            attn(prefix + "ca.", l.crossattention)
        out[prefix + "f1.w"], out[prefix + "f1.b"] = l.intermediate.dense.weight, l.intermediate.dense.bias
        out[prefix + "f2.w"], out[prefix + "f2.b"] = l.output.dense.weight, l.output.dense.bias
        out[prefix + "ln2.w"], out[prefix + "ln2.b"] = l.output.LayerNorm.weight, l.output.LayerNorm.bias

    emb("enc.emb.", model.encoder.embeddings)
    for i, l in enumerate(model.encoder.encoder.layer):
        layer(f"enc.{i}.", l, False)
    emb("dec.emb.", model.decoder.bert.embeddings)
    for i, l in enumerate(model.decoder.bert.encoder.layer):
        layer(f"dec.{i}.", l, True)
    h = model.decoder.cls.predictions
    out["head.t.w"], out["head.t.b"] = h.transform.dense.weight, h.transform.dense.bias
    out["head.ln.w"], out["head.ln.b"] = h.transform.LayerNorm.weight, h.transform.LayerNorm.bias
    out["head.bias"] = h.decoder.bias
    assert h.decoder.weight is out["dec.emb.word"], "the LM head must be tied to the decoder word table"
    if hasattr(model, "vector_quantizer"):
        out["vq.E"] = model.vector_quantizer.embedding.weight
    return out


def site_keys(n_enc, n_dec):
    """Every dropout of the step, in forward order, as (key, kind) with kind "emb" | "attn" | "hid"."""
    keys = [("enc.emb", "emb")]
    for i in range(n_enc):
        keys += [(f"enc.{i}.sa.attn", "attn"), (f"enc.{i}.sa.out", "hid"), (f"enc.{i}.ffn", "hid")]
    keys.append(("dec.emb", "emb"))
    for i in range(n_dec):
        keys += [(f"dec.{i}.sa.attn", "attn"), (f"dec.{i}.sa.out", "hid"), (f"dec.{i}.ca.attn", "attn"),
                 (f"dec.{i}.ca.out", "hid"), (f"dec.{i}.ffn", "hid")]
    return keys


def attend_allowed(B, Sq, Sk, key_mask, causal, device):
    """[B, 1, Sq, Sk] bool: which (query, key) pairs attend -- key_mask [B, Sk] (1 = attend) or None, causal = key <= query."""
    allow = torch.ones(B, 1, Sq, Sk, dtype=torch.bool, device=device)
    if key_mask is not None:
        allow = allow & key_mask.bool().to(device)[:, None, None, :]
    if causal:
        allow = allow & torch.ones(Sq, Sk, dtype=torch.bool, device=device).tril()[None, None]
    return allow


def masked_softmax(s, allow, empty_rows_zero=False):
    """softmax over the keys of scaled scores s with the additive mask of BertSelfAttention (-inf where a pair does not attend).
    A query row without any attended key is NaN in torch; empty_rows_zero defines it as all-zero probabilities (and a zero
    gradient), which is what the HIP kernels compute there (include/kvq.h, kvq_attn_fwd)."""
    if not empty_rows_zero:
        return torch.softmax(s.masked_fill(~allow, float("-inf")), -1)
    some = allow.any(-1, keepdim=True)
    return torch.softmax(s.masked_fill(~allow & some, float("-inf")), -1) * some.to(s.dtype)


def dropout_scale(x, keep, p):
    """x * keep / (1 - p): `keep` a 0 / 1 tensor of x's shape."""
    return x * (keep.to(device=x.device, dtype=x.dtype) / (1.0 - p))


def ref_step(W, ids, mask, nh, eps=1e-12, dec_ids=None, dec_mask=None, target=None, idx=None, beta=0.25, keep=None,
             p_hid=0.0, p_attn=0.0, pad_idx=0, dtype=torch.float64):
    """One step of the model whose parameters are W {engine name: tensor} (any device / dtype; upcast to `dtype`).
    idx: the code index of every encoder token ([N] or [B, S, 1]) -- required when W holds "vq.E".
    Returns dict(loss_recon, loss_vq (None for Bagon), logits [B, Sd, V], z (encoder output [N, H]), grads {name: tensor})."""
    keep = keep or {}
    P = {n: w.detach().to(dtype).clone().requires_grad_(True) for n, w in W.items()}
    n_enc = 1 + max(int(n.split(".")[1]) for n in P if n.startswith("enc.") and n.split(".")[1].isdigit())
    n_dec = 1 + max(int(n.split(".")[1]) for n in P if n.startswith("dec.") and n.split(".")[1].isdigit())
    B, S = ids.shape
    d_ids = ids if dec_ids is None else dec_ids
    d_mask = mask if dec_mask is None else dec_mask
    Sd = d_ids.shape[1]
    tgt = d_ids if target is None else target
    H = P["enc.emb.word"].shape[1]
    dh = H // nh

    def drop(x, key, p):
        k = keep.get(key)
        if k is None:
            return x
        assert tuple(k.shape) == tuple(x.shape), (key, tuple(k.shape), tuple(x.shape))
        return dropout_scale(x, k, p)

    def ln(x, pre):
        return F.layer_norm(x, (H,), P[pre + ".w"], P[pre + ".b"], eps)

    def embeddings(pre, t, key):
        Bt, St = t.shape
        x = F.embedding(t, P[pre + "word"], padding_idx=pad_idx) + P[pre + "pos"][:St] + P[pre + "type"][0]
        return drop(ln(x.reshape(Bt * St, H), pre + "ln"), key, p_hid)

    def attention(pre, x, kv, key_mask, causal, Sq, Sk, key):
        src = x if kv is None else kv
        q = F.linear(x, P[pre + "q.w"], P[pre + "q.b"]).view(B, Sq, nh, dh).transpose(1, 2)
        k = F.linear(src, P[pre + "k.w"], P[pre + "k.b"]).view(B, Sk, nh, dh).transpose(1, 2)
        v = F.linear(src, P[pre + "v.w"], P[pre + "v.b"]).view(B, Sk, nh, dh).transpose(1, 2)
        s = q @ k.transpose(-1, -2) / math.sqrt(dh)
        pr = drop(masked_softmax(s, attend_allowed(B, Sq, Sk, key_mask, causal, x.device)), key, p_attn)
        return (pr @ v).transpose(1, 2).reshape(B * Sq, H)

    def out_block(pre, wname, h, resid, key, lnname):
        y = F.linear(h, P[pre + wname + ".w"], P[pre + wname + ".b"])
        return ln(drop(y, key, p_hid) + resid, pre + lnname)

    def layer(pre, x, key_mask, causal, Sq, enc=None):
        a = attention(pre + "sa.", x, None, key_mask, causal, Sq, Sq, pre[:-1] + ".sa.attn")
        x = out_block(pre + "sa.", "o", a, x, pre[:-1] + ".sa.out", "ln")
        if enc is not None:
            c = attention(pre + "ca.", x, enc, None, False, Sq, S, pre[:-1] + ".ca.attn")
            x = out_block(pre + "ca.", "o", c, x, pre[:-1] + ".ca.out", "ln")
        h = F.gelu(F.linear(x, P[pre + "f1.w"], P[pre + "f1.b"]))
        return out_block(pre, "f2", h, x, pre[:-1] + ".ffn", "ln2")

    x = embeddings("enc.emb.", ids, "enc.emb")
    for i in range(n_enc):
        x = layer(f"enc.{i}.", x, mask, False, S)
    z = x
    loss_vq = None
    if "vq.E" in P:
        assert idx is not None, "a Shelgon step needs the code indices"
        zq = P["vq.E"][idx.reshape(-1).to(z.device)]
        loss_vq = torch.mean((zq.detach() - z) ** 2) + beta * torch.mean((zq - z.detach()) ** 2)     # VectorQuantizer.py:76-77
        enc = z + (zq - z).detach()                                                                  # :80
    else:
        enc = z
    y = embeddings("dec.emb.", d_ids, "dec.emb")
    for i in range(n_dec):
        y = layer(f"dec.{i}.", y, d_mask, True, Sd, enc)
    t = F.gelu(F.linear(y, P["head.t.w"], P["head.t.b"]))
    logits = F.linear(ln(t, "head.ln"), P["dec.emb.word"], P["head.bias"])
    loss_recon = F.cross_entropy(logits, tgt.reshape(-1).to(logits.device))
    total = loss_recon + loss_vq if loss_vq is not None else loss_recon
    total.backward()
    return dict(loss_recon=loss_recon.detach(), loss_vq=loss_vq.detach() if loss_vq is not None else None,
                logits=logits.detach().view(B, Sd, -1), z=z.detach(),
                grads={n: p.grad if p.grad is not None else torch.zeros_like(p) for n, p in P.items()})
