"""The inference side of TrainEngine: attention maps, the latent analyses (encode / decode / traverse_codes), free-running
generation, beam search, sampling and the reconstruction metrics (DESIGN.md sections 5i-5l).

InferenceMixin holds the methods and nothing else: TrainEngine (kvq/engine.py) inherits it, owns every attribute they read -- the
flat buffers, forward_backward and the layer helpers of the training schedule, the two caches self._gen_cache / self._beam_cache --
and runs none of them inside the training step.  This module does not import kvq.engine.
"""
from __future__ import annotations

import math

import torch

from . import nnops
from ._ffi import KvqError, check, lib


def _round_up(x, a):
    return (x + a - 1) // a * a


class SamplingRefused(KvqError, TypeError):
    """A sampling argument (top_k, top_p, temperature, seed, want_scores) handed to beam search: a KvqError naming the argument;
    a TypeError as well, which is what an unknown keyword is."""


class InferenceMixin:
    _MAP_FAMILY = {("enc", "sa"): "enc_self", ("dec", "sa"): "dec_self", ("dec", "ca"): "cross"}

    def _maps_emit(self, pre, q, k, v, mask, causal, B, Sq, Sk, lse):
        """attention_maps(): the probabilities of the attention block `pre` ("dec.1.ca."), from launches of their own on the
        block's q / k views and mask -- into the census' table of (family, layer) and / or the per-sentence stack."""
        side, layer, kind = pre.split(".")[:3]
        family = self._MAP_FAMILY[(side, kind)]
        m = self._maps
        if family not in m["families"]:
            return
        layer = int(layer)
        probs = m["per_sentence"][family][layer] if m["per_sentence"] is not None else None
        table = m["census"].tables[family][layer] if m["census"] is not None else None
        nnops.attn_probs(q, k, v, mask, B, self.nh, Sq, Sk, causal, lse=lse if max(Sq, Sk) > 32 else None, probs=probs, table=table)

    def attention_maps(self, enc_ids, enc_mask, dec_ids=None, dec_mask=None, census=None, per_sentence=False):
        """The attention probabilities of an evaluation forward (no dropout, quantiser in eval mode, eager; the schedule of
        forward_logits) -- what HuggingFace returns as `attentions` / `cross_attentions` under output_attentions=True, which
        analyses/cross_attention/extract_model_cross_attention.py:79-86 stacks and averages on the host.  Families: "dec_self"
        (causal, decoder mask), "cross" (no key mask: models/bagon/Bagon.py:50-53 passes none), "enc_self"; those of `census`, or
        the decoder's two without one.
        census: a kvq.census.AttentionCensus -- every asked-for block adds the sum over this batch's sentences into its f64 table
        on the device; nothing of size B is kept.  per_sentence: also return {family: f32 [L, B, nh, Sq, Sk]}, i.e.
        torch.stack(decoder_output.cross_attentions) etc.  The maps come from kernels of their own (kvq_attn_probs) after each
        block's forward kernel: the training step and forward_logits launch exactly what they launched before."""
        if census is None and not per_sentence:
            raise KvqError("TrainEngine.attention_maps: pass a census, per_sentence=True, or both")
        if self._cap is not None or torch.cuda.is_current_stream_capturing():
            raise KvqError("TrainEngine.attention_maps is an eager call: not under graph capture")
        if self.group is not None or self._dp:
            raise KvqError("TrainEngine.attention_maps is a single-process call (this engine has a process group)")
        families = tuple(census.families) if census is not None else ("dec_self", "cross")
        B, Se = enc_ids.shape
        Sd = Se if dec_ids is None else dec_ids.shape[1]
        dims = {"enc_self": (self.n_enc_layers, Se, Se), "dec_self": (self.n_dec_layers, Sd, Sd), "cross": (self.n_dec_layers, Sd, Se)}
        if census is not None:
            for f in families:             # before anything is launched: a table that does not fit must not leave half a batch behind
                census.require(f, dims[f][0], self.nh, dims[f][1], dims[f][2], self.dev)
        stacks = None
        if per_sentence:
            stacks = {f: torch.empty((dims[f][0], B, self.nh, dims[f][1], dims[f][2]), dtype=torch.float32, device=self.dev)
                      for f in families}
        self.refresh_if_params_changed()
        self._distrust_codebook_pack()
        self._maps = dict(families=families, census=census, per_sentence=stacks)
        try:
            self.forward_backward(enc_ids, enc_mask, training=False, compute_grads=False, dec_ids=dec_ids, dec_mask=dec_mask,
                                  quantizer_training=False)
        finally:
            self._maps = None
        if census is not None:
            census.count += B
        return stacks

    # ------------------------------------------------------------------------------------------------------------
    # latent analyses: the schedule of forward_logits entered / left at the latent (evaluation mode, eager, one process)
    # ------------------------------------------------------------------------------------------------------------
    _TRAVERSE_CHUNK = 256               # variants per decode of traverse_codes

    def _latent_call(self, what, refresh=True):
        """What encode / decode / decode_codes / traverse_codes refuse, before anything is launched.  refresh=False: the refusals
        alone (generate runs them in front of its argument checks, which read the prompt's range from the device)."""
        if self._cap is not None or torch.cuda.is_current_stream_capturing():
            raise KvqError(f"TrainEngine.{what} is an eager call: not under graph capture")
        if self.group is not None or self._dp:
            raise KvqError(f"TrainEngine.{what} is a single-process call (this engine has a process group)")
        if self.fp8:
            raise KvqError(f"TrainEngine.{what}: not on an fp8 engine -- its GEMMs read fp8 copies that the kernel producing an "
                           f"activation writes beside it, and a latent handed in from outside has no such producer-written copy")
        if not refresh:
            return
        self.refresh_if_params_changed()
        self._distrust_codebook_pack()

    def _seq_limit(self, what, *lengths):
        lim = 128 if self.dtype == torch.bfloat16 else 32
        if max(lengths) > lim:
            raise KvqError(f"TrainEngine.{what}: sequence length {max(lengths)} above the attention kernels' limit ({lim} tokens "
                           f"in {'bf16' if lim == 128 else 'f32'})")

    def encode(self, enc_ids, enc_mask, quantize=True):
        """The latent of a batch: dict(z [B, S, H] = the encoder's output in the engine's dtype) and, for a model with a quantiser
        and quantize=True, z_q [B, S, H], indices (as forward_logits returns them), perplexity, loss_vq_raw -- the quantiser in
        evaluation mode.  What analyses/latent_arithmetics/latent_arithmetics_Bagon.py:92 takes from the HF encoder and
        analyses/latent_traversals/latent_traversals_Shelgon_latent_classes.py:120-126 from encoder + quantiser."""
        self._latent_call("encode")
        if enc_ids.dim() != 2 or enc_mask.shape != enc_ids.shape:
            raise KvqError("TrainEngine.encode: enc_ids [B, S] needs an enc_mask of its shape")
        self._seq_limit("encode", enc_ids.shape[1])
        if self.has_vq and quantize:
            return self.forward_backward(enc_ids, enc_mask, training=False, compute_grads=False, quantizer_training=False,
                                         stop_after_quantizer=True, want_latents=True)
        return self.forward_backward(enc_ids, enc_mask, training=False, compute_grads=False, stop_after_encoder=True)

    def decode(self, latents, dec_ids, dec_mask, target_ids=None, quantize=False, want_logits=False):
        """The decoder and LM head of forward_logits on a latent of the caller's choosing: latents [B, Se, H] (the engine's dtype,
        contiguous) is the cross-attention source (HF's encoder_hidden_states, latent_arithmetics_Bagon.py:133-137); Se may differ
        from the decoder's length.  quantize=True sends the latents through the quantiser (evaluation mode) first -- the caller
        edits z -- and the result then carries `indices`.  Returns dict(recon_ids [B, Sd], acc, acc_per_sentence [B], loss_recon
        [, logits [B, Sd, V]] [, indices]), scored against target_ids (default: dec_ids) by the kvq_ce_forward path."""
        self._latent_call("decode")
        if not torch.is_tensor(latents) or latents.dim() != 3 or latents.shape[2] != self.H:
            raise KvqError(f"TrainEngine.decode: latents must be [B, Se, {self.H}], got "
                           f"{tuple(latents.shape) if torch.is_tensor(latents) else type(latents).__name__}")
        if latents.dtype != self.dtype or latents.device != self.dev or not latents.is_contiguous():
            raise KvqError(f"TrainEngine.decode: latents must be contiguous {self.dtype} on {self.dev}, got {latents.dtype} on {latents.device}")
        if dec_ids.dim() != 2 or dec_ids.shape[0] != latents.shape[0]:
            raise KvqError(f"TrainEngine.decode: {latents.shape[0]} latents but dec_ids {tuple(dec_ids.shape)}")
        if dec_mask is None or dec_mask.shape != dec_ids.shape:
            raise KvqError("TrainEngine.decode: dec_ids needs a dec_mask of its shape")
        if quantize and not self.has_vq:
            raise KvqError("TrainEngine.decode: quantize=True, but the model has no quantiser")
        self._seq_limit("decode", latents.shape[1], dec_ids.shape[1])
        out = self.forward_backward(None, None, training=False, compute_grads=False, dec_ids=dec_ids, dec_mask=dec_mask,
                                    want_logits=want_logits, quantizer_training=False, target_ids=target_ids, latents=latents,
                                    skip_quantizer=not quantize)
        res = {k: out[k] for k in ("recon_ids", "acc", "acc_per_sentence", "loss_recon") + (("loss_tokens",) if "loss_tokens" in out else ())}
        if want_logits:
            res["logits"] = out["logits"]
        if quantize:
            res["indices"] = out["indices"]
        return res

    def _code_rows(self, what, indices):
        """indices [B, Se] / [B, Se, G] int64 -> the contiguous [B, Se, G] the lookup kernel reads."""
        if self.vq_kind not in ("VectorQuantizer", "MultiVectorQuantizer"):
            raise KvqError(f"TrainEngine.{what}: needs a VectorQuantizer or MultiVectorQuantizer codebook (this model has "
                           f"{self.vq_kind or 'no quantiser'})")
        if not torch.is_tensor(indices) or indices.dtype != torch.int64 or indices.device != self.dev:
            raise KvqError(f"TrainEngine.{what}: indices must be an int64 tensor on {self.dev}")
        if indices.dim() == 2 and self.G == 1:
            indices = indices.unsqueeze(-1)
        if indices.dim() != 3 or indices.shape[2] != self.G:
            raise KvqError(f"TrainEngine.{what}: indices must be [B, Se, {self.G}]" + (" or [B, Se]" if self.G == 1 else "")
                           + f", got {tuple(indices.shape)}")
        return indices.contiguous()

    def codes_to_latents(self, indices):
        """z_q [B, Se, H] in the engine's dtype = the codebook rows of indices [B, Se] / [B, Se, G] (kvq_vq_lookup): the row itself,
        not the straight-through value the quantiser's forward hands on.  An index outside [0, K) raises."""
        idx = self._code_rows("codes_to_latents", indices)
        B, Se, G = idx.shape
        bad = torch.zeros(1, dtype=torch.int32, device=self.dev)
        rows = nnops.vq_lookup(idx.view(B * Se, G), self.E.data, self.K, self.dtype, n_bad=bad)
        if int(bad.item()):
            raise KvqError(f"TrainEngine.codes_to_latents: {int(bad.item())} indices outside [0, {self.K})")
        vq = self.model.vector_quantizer
        if getattr(vq, "ragged", False):             # padded slices back to the e_dim columns (MultiVectorQuantizer.merge)
            rows = rows.index_select(1, vq.inv_map)
        return rows.view(B, Se, self.H)

    def decode_codes(self, indices, dec_ids, dec_mask, target_ids=None, want_logits=False):
        """decode() of the codebook rows of `indices` [B, Se] / [B, Se, G] int64: what
        latent_traversals_Shelgon_latent_classes.py:139-150 does after overwriting the discrete latent by hand."""
        self._latent_call("decode_codes")
        return self.decode(self.codes_to_latents(indices), dec_ids, dec_mask, target_ids=target_ids, want_logits=want_logits)

    # ------------------------------------------------------------------------------------------------------------
    # free-running generation: the decoder one position at a time over a key/value cache
    # ------------------------------------------------------------------------------------------------------------
    _GEN_GRAPHS_KEPT = 8                # captured steps kept per engine (one per shape / choice rule), oldest dropped first

    @classmethod
    def _check_generate(cls, latents, max_length, prompt_ids, H, dtype, dev, pos_rows, temperature, **ids_kw):
        """The argument checks of generate() that need no device: every refusal happens before any launch."""
        if not torch.is_tensor(latents) or latents.dim() != 3 or latents.shape[2] != H:
            raise KvqError(f"TrainEngine.generate: latents must be [B, Se, {H}], got "
                           f"{tuple(latents.shape) if torch.is_tensor(latents) else type(latents).__name__}")
        if latents.dtype != dtype or latents.device != dev or not latents.is_contiguous():
            raise KvqError(f"TrainEngine.generate: latents must be contiguous {dtype} on {dev}, got {latents.dtype} on {latents.device}")
        if latents.shape[0] < 1 or latents.shape[1] < 1:
            raise KvqError(f"TrainEngine.generate: empty latents {tuple(latents.shape)}")
        cls._check_generate_call(latents.shape[0], max_length, prompt_ids, dev, pos_rows, temperature, **ids_kw)

    @staticmethod
    def _check_generate_call(B, max_length, prompt_ids, dev, pos_rows, temperature, V=None, eos_id=None, pad_id=None, seed=0):
        """The part of _check_generate that does not look at the latents (generate_codes runs it before the codebook lookup).
        V (the vocabulary size): eos_id, pad_id and every prompt id must be token ids; the prompt's range is one reduction over
        [B, P] and a host read, the only device work of the checks."""
        if isinstance(max_length, bool) or not isinstance(max_length, int) or max_length < 1:
            raise KvqError(f"TrainEngine.generate: max_length must be a positive int, got {max_length!r}")
        if max_length > pos_rows:
            raise KvqError(f"TrainEngine.generate: max_length {max_length} above the decoder's position table ({pos_rows} rows)")
        if not torch.is_tensor(prompt_ids) or prompt_ids.dtype != torch.int64 or prompt_ids.dim() != 2 \
                or prompt_ids.shape[0] != B or prompt_ids.shape[1] < 1:
            raise KvqError(f"TrainEngine.generate: prompt_ids must be int64 [B, P] with B = {B} and P >= 1 (e.g. a column "
                           f"of start ids), got {tuple(prompt_ids.shape) if torch.is_tensor(prompt_ids) else type(prompt_ids).__name__}"
                           + (f" {prompt_ids.dtype}" if torch.is_tensor(prompt_ids) else ""))
        if prompt_ids.device != dev:
            raise KvqError(f"TrainEngine.generate: prompt_ids must be on {dev}, got {prompt_ids.device}")
        if prompt_ids.shape[1] > max_length:
            raise KvqError(f"TrainEngine.generate: a prompt of {prompt_ids.shape[1]} tokens does not fit max_length {max_length}")
        if not (float(temperature) >= 0.0) or float(temperature) == float("inf") or (temperature > 0 and 1.0 / float(temperature) > 3.0e38):
            raise KvqError(f"TrainEngine.generate: temperature must be finite and >= 0 (0 = greedy; 1 / temperature an f32), got {temperature!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < (1 << 64):
            raise KvqError(f"TrainEngine.generate: seed must be an int in [0, 2^64), got {seed!r}")
        for name, v in (("eos_id", eos_id), ("pad_id", pad_id)):
            if v is not None and (isinstance(v, bool) or not isinstance(v, int) or v < 0 or (V is not None and v >= V)):
                raise KvqError(f"TrainEngine.generate: {name} must be None or a token id (an int in [0, {V if V is not None else 'V'})), got {v!r}")
        if V is not None:
            lo, hi = (int(x) for x in torch.aminmax(prompt_ids))
            if lo < 0 or hi >= V:
                raise KvqError(f"TrainEngine.generate: prompt_ids hold ids outside [0, {V}) (smallest {lo}, largest {hi})")

    @staticmethod
    def _check_filters(top_k, top_p, temperature, want_scores, V=None):
        """What generate() refuses about top_k / top_p / want_scores; needs no device.  -> whether the filtered selection runs."""
        if isinstance(top_k, bool) or not isinstance(top_k, int) or not 0 <= top_k < (1 << 31):
            raise KvqError(f"TrainEngine.generate: top_k must be an int >= 0 (0 = off), got {top_k!r}")
        if isinstance(top_p, bool) or not isinstance(top_p, (int, float)) or not (0.0 < float(top_p) <= 1.0):
            raise KvqError(f"TrainEngine.generate: top_p must be a finite number in (0, 1] (1 = off), got {top_p!r}")
        filtered = top_k != 0 or float(top_p) != 1.0
        if filtered and not float(temperature) > 0.0:
            raise KvqError(f"TrainEngine.generate: top_k / top_p change nothing at temperature 0 (the arg-max is in every kept set): "
                           f"got top_k={top_k!r}, top_p={top_p!r} with temperature={temperature!r}")
        if (filtered or want_scores) and V is not None and V > nnops.GEN_FILTER_MAX_V:
            raise KvqError(f"TrainEngine.generate: top_k / top_p / want_scores need a vocabulary of at most {nnops.GEN_FILTER_MAX_V} "
                           f"words (kvq_gen_select_filtered holds a row in registers), this decoder has {V}")
        return bool(filtered or want_scores)

    _SAMPLING_DEFAULTS = dict(top_k=0, top_p=1.0, temperature=0.0, seed=0, want_scores=False)
    _SAMPLING_KEYS = tuple(_SAMPLING_DEFAULTS)

    @classmethod
    def _refuse_sampling(cls, who, kw, why="beam search is deterministic and takes no {} (sampling belongs to generate(); sampled "
                                           "beams are not supported)"):
        """beam_search takes no sampling argument (sampled beams are out of scope): a KvqError naming them -- one that is also the
        TypeError such a keyword raised while beam_search had no **kw, so a caller written against either catches it.  `why`: the
        sentence of the caller, the names go where its {} is."""
        given = [k for k in cls._SAMPLING_KEYS if k in kw]
        if given:
            raise SamplingRefused(f"TrainEngine.{who}: " + why.format(", ".join(given)))
        if kw:
            raise TypeError(f"TrainEngine.{who}() got an unexpected keyword argument {next(iter(kw))!r}")

    def _gen_step(self, g):
        """One position: the decoder layer schedule of _fb_gen on [R, H] rows, the token at column t in, the token at t + 1 out.
        Launches only (no host read): the body of the captured graph, and what graph=False runs max_length - 1 times.
        With g["W"] (beam_search: the rows are slot space) the two attention calls follow the ancestry
        table and the selection is a step of the search; everything else is the same launch on R rows."""
        fl, H, nh, dcfg = self.flat, self.H, self.nh, self.dcfg
        eps, st, W = dcfg.layer_norm_eps, g["state"], g.get("W")
        x = nnops.gen_embed(st, g["ids"], fl.w("dec.emb.word"), fl.w("dec.emb.pos"), fl.w("dec.emb.type")[0], fl.w32("dec.emb.ln.w"),
                            fl.w32("dec.emb.ln.b"), eps)
        for i in range(self.n_dec_layers):
            pre = f"dec.{i}.sa."
            qkv = self._linear(x, None, None, fused=([pre + "q.w", pre + "k.w", pre + "v.w"], [pre + "q.b", pre + "k.b", pre + "v.b"]))
            if W is None:
                ctx = nnops.gen_attn_self(st, qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], g["cache"][i], nh)
            else:
                ctx = nnops.beam_attn_self(st, qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], g["cache"][i], g["anc"], nh)
            x = self._dense_residual_ln(ctx, pre + "o.w", pre + "o.b", x, pre + "ln.w", pre + "ln.b", eps, 0.0, 0)[0]
            pre = f"dec.{i}.ca."
            q = self._linear(x, pre + "q.w", pre + "q.b")
            ctx = nnops.gen_attn_cross(st, q, g["kv"][i], g["Se"], nh) if W is None else nnops.beam_attn_cross(st, q, g["kv"][i], g["Se"], nh, W)
            x = self._dense_residual_ln(ctx, pre + "o.w", pre + "o.b", x, pre + "ln.w", pre + "ln.b", eps, 0.0, 0)[0]
            pre = f"dec.{i}."
            a = self._linear_gelu(x, pre + "f1.w", pre + "f1.b")[1]
            x = self._dense_residual_ln(a, pre + "f2.w", pre + "f2.b", x, pre + "ln2.w", pre + "ln2.b", eps, 0.0, 0)[0]
        ta = self._linear_gelu(x, "head.t.w", "head.t.b")[1]
        hN = nnops.ln_fwd(ta, None, fl.w32("head.ln.w"), fl.w32("head.ln.b"), eps, save_pre=False)[0]
        Wv = fl.w("dec.emb.word", rows=self.Vp)
        bv = fl.shadow[fl.seg["head.bias"][0]: fl.seg["head.bias"][0] + self.Vp]
        logits = self._linear(hN, None, None, Wb=(Wv, bv), key="dec.emb.word")                      # [R, Vp]
        if W is None and g.get("filter") is not None:       # (top_k, top_p: in the filter state, as temperature and seed in st)
            nnops.gen_select_filtered(st, g["filter"], logits, self.V, g["ids"], g["finished"], g["lengths"], g["step_logits"], g["kept"],
                                      g["cut"], g["logprob"])
        elif W is None:
            nnops.gen_select(st, logits, self.V, g["ids"], g["finished"], g["lengths"], g["step_logits"])  # (temperature, seed: in the state)
        else:
            nnops.beam_select(st, logits, self.V, W, g["ids"], g["parent"], g["scores"], g["step_scores"], g["anc"], g["finished"],
                              g["lengths"], g["step_logits"])
        nnops.gen_advance(st)

    def _gen_buffers(self, B, Se, L, want_logits, graph, filtered=False, W=None):
        """The buffers of one (B, Se, max_length) -- allocated once, the same addresses in every call -- and, with graph, the captured
        step: position, prompt length, end token, temperature and seed all live in the device state, so one graph serves every call
        of the shape.  Kept per engine and kind of call, the oldest of more than _GEN_GRAPHS_KEPT is dropped.
        W = None (generate): R = round_up(B, 8) rows, a latent each (S = R).  W beams (beam_search): beam w of
        sentence b is row b W + w of R = round_up(B W, 8) rows of slot space; S = ceil(R / W) sentences of latents (zero behind B:
        the pad rows read valid memory), the ancestry and score tensors, and _gen_step runs the search with g["W"].
        filtered: the variant whose step selects with kvq_gen_select_filtered (top_k and top_p in a filter state of its own),
        under a key of its own."""
        cache = self._gen_cache if W is None else self._beam_cache
        key = (B, Se, L) + (() if W is None else (W,)) + (bool(want_logits), self.flat.shadow.data_ptr()) + (("filtered",) if filtered else ())
        g = cache.get(key)
        if g is None:
            dev, H, nl, w = self.dev, self.H, self.n_dec_layers, W or 1
            R = _round_up(B * w, 8)
            S = -(-R // w)
            g = dict(B=B, R=R, S=S, Se=Se, L=L, graph=None, replays=0,
                     state=nnops.new_gen_state(dev, 0, 1, L, None, 0),
                     ids=torch.zeros((R, L), dtype=torch.int64, device=dev),
                     finished=torch.zeros(R, dtype=torch.int32, device=dev), lengths=torch.zeros(R, dtype=torch.int32, device=dev),
                     cache=[torch.zeros((R, L, 2 * H), dtype=self.dtype, device=dev) for _ in range(nl)],
                     lat=torch.zeros((S, Se, H), dtype=self.dtype, device=dev),
                     step_logits=torch.zeros((R, L, self.V), dtype=torch.float32, device=dev) if want_logits else None)
            if W is not None:
                g.update(W=W, hyp=torch.zeros((R, L), dtype=torch.int64, device=dev),
                         own=torch.arange(R, dtype=torch.int32, device=dev).view(R, 1).expand(R, L).contiguous(),
                         parent=torch.zeros((R, L), dtype=torch.int32, device=dev), anc=torch.zeros((2, R, L), dtype=torch.int32, device=dev),
                         scores=torch.zeros(R, dtype=torch.float32, device=dev), step_scores=torch.zeros((R, L), dtype=torch.float32, device=dev))
            if filtered:
                g.update(filter=nnops.new_gen_filter(dev), kept=torch.zeros((R, L), dtype=torch.int32, device=dev),
                         cut=torch.zeros((R, L), dtype=torch.int32, device=dev), logprob=torch.zeros((R, L), dtype=torch.float32, device=dev))
            if self._cakv_batched:
                g["kv_all"] = torch.empty((S * Se, nl * 2 * H), dtype=self.dtype, device=dev)
                g["kv"] = [g["kv_all"][:, 2 * H * i: 2 * H * (i + 1)] for i in range(nl)]
            else:
                g["kv"] = [torch.empty((S * Se, 2 * H), dtype=self.dtype, device=dev) for _ in range(nl)]
            while len(cache) >= self._GEN_GRAPHS_KEPT:
                cache.pop(next(iter(cache)))
            cache[key] = g
        if graph and g["graph"] is None and L > 1:
            if W is not None:                       # (generate's first step runs on the zeroed buffers as they are)
                self._gen_reset(g, 1, None, 0)
            self._gen_step(g)                       # once eagerly: whatever a library allocates on first use happens outside the capture
            g["graph"] = self._gen_capture(g)
        return g

    def _gen_capture(self, g):
        """The step as ONE hipGraph, captured on a single stream (no parallel branches); kernel nodes only (gen_census)."""
        import gc
        dev = self.dev
        graph = torch.cuda.CUDAGraph(keep_graph=True)
        side = torch.cuda.Stream(device=dev)
        gc_was_on = gc.isenabled()
        try:
            gc.collect()
            gc.disable()                            # (as _StepGraphs: no HIP object may be destroyed while this thread captures)
            torch.cuda.synchronize(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                graph.capture_begin(capture_error_mode="thread_local")
                try:
                    self._gen_step(g)
                finally:
                    graph.capture_end()
        finally:
            if gc_was_on:
                gc.enable()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        return graph

    def gen_census(self):
        """Per captured generation step (generate's, then beam_search's): {kind: nodes} (kvq_graph_census), as _StepGraphs.node_census."""
        import ctypes
        kinds = ("kernel", "memset", "memcpy", "empty", "event", "other")
        out = []
        for g in list(self._gen_cache.values()) + list(self._beam_cache.values()):
            if g["graph"] is not None:
                counts = (ctypes.c_int64 * len(kinds))()
                check(lib().kvq_graph_census(g["graph"].raw_cuda_graph(), counts), "kvq_graph_census")
                out.append(dict(zip(kinds, (int(c) for c in counts))))
        return out

    def _gen_reset(self, g, P, eos_id, pad, prompt_ids=None, temperature=0.0, seed=0):
        """The start of a call: position 0 and the call's constants in the state words, pads behind the prompt, every live row
        unfinished, the rows that pad the batch to a multiple of 8 finished (computed, never reported)."""
        L, W = g["L"], g.get("W")
        n = g["B"] * (W or 1)
        g["state"].copy_(torch.tensor(nnops.gen_state_words(0, P, L, eos_id, pad, temperature, seed), dtype=torch.int32), non_blocking=False)
        g["ids"].fill_(pad)
        if prompt_ids is not None:
            g["ids"][:n, :P].copy_(prompt_ids if W is None else prompt_ids.repeat_interleave(W, dim=0))
        if W is not None:
            self._beam_reset(g)
        g["finished"].zero_()
        g["finished"][n:].fill_(1)
        g["lengths"].fill_(L)
        if g["step_logits"] is not None:
            g["step_logits"].zero_()

    def _beam_reset(self, g):
        """What the start of a search sets beyond _gen_reset: every history the identity, beam 0 of a sentence alive with score 0
        and the others dead (-inf: the first free step then draws W distinct tokens from one row), the rows behind B W dead."""
        g["anc"].copy_(g["own"].unsqueeze(0).expand(2, -1, -1))
        g["parent"].copy_(g["own"])
        g["step_scores"].zero_()
        g["scores"].fill_(float("-inf"))
        g["scores"][:g["B"] * g["W"]:g["W"]].zero_()

    def _quantized(self, latents, res):
        """quantize=True of generate / beam_search: the latents through the quantiser in evaluation mode, as decode(quantize=True);
        the indices into res."""
        B, Se, _ = latents.shape
        one = torch.zeros((B, 1), dtype=torch.int64, device=self.dev)
        q = self.forward_backward(None, None, training=False, compute_grads=False, dec_ids=one, dec_mask=torch.ones_like(one),
                                  quantizer_training=False, stop_after_quantizer=True, want_latents=True, latents=latents)
        res["indices"] = q["indices"]
        return q["z_q"].reshape(B, Se, self.H)

    def _gen_run(self, g, latents, prompt_ids, eos_id, pad_id, graph, temperature=0.0, seed=0, filter_words=None):
        """A call on the buffers g: once, the cross-attention keys | values of every layer (once per SENTENCE in a search) and the
        start state; then max_length - 1 steps, replayed or eager, with no host read."""
        B, Se, L, fl = g["B"], g["Se"], g["L"], self.flat
        g["lat"][:B].copy_(latents)
        lat = g["lat"].view(g["S"] * Se, self.H)
        if self._cakv_batched:
            g["kv_all"].copy_(self._linear(lat, None, None, Wb=(fl.fused(self._cakv_w, fl.shadow), fl.fused(self._cakv_b, fl.shadow)),
                                           key=self._cakv_w[0]))
        else:
            for i in range(self.n_dec_layers):
                pre = f"dec.{i}.ca."
                g["kv"][i].copy_(self._linear(lat, None, None, fused=([pre + "k.w", pre + "v.w"], [pre + "k.b", pre + "v.b"])))
        pad = (self._pad_idx if self._pad_idx is not None else 0) if pad_id is None else int(pad_id)
        self._gen_reset(g, prompt_ids.shape[1], eos_id, pad, prompt_ids, temperature, seed)
        if filter_words is not None:
            g["filter"].copy_(torch.tensor(filter_words, dtype=torch.int32), non_blocking=False)
            g["kept"].zero_()
            g["cut"].zero_()
            g["logprob"].zero_()
        for _ in range(L - 1):
            if graph:
                g["graph"].replay()
            else:
                self._gen_step(g)
        g["replays"] += (L - 1) if graph else 0

    def generate(self, latents, max_length, prompt_ids, eos_id=None, pad_id=None, temperature=0.0, seed=0, quantize=False,
                 want_logits=False, graph=True, top_k=0, top_p=1.0, want_scores=False):
        """Free-running generation from a latent: the decoder sees only the prompt and what it has written itself.  latents
        [B, Se, H] as decode() takes them; prompt_ids [B, P] int64 (P >= 1, e.g. a column of start ids) fills columns 0 .. P-1, the
        recurrence  ids[:, t + 1] = choose(logits(latents, ids[:, :t + 1])[t])  the rest up to max_length.  choose: the first arg-max
        (temperature 0) or a draw from softmax(logits / temperature) (kvq_gen_select; `seed`).  A sentence that chooses eos_id is
        finished: lengths = its tokens including the end token, pad_id (default: the embeddings' padding_idx, else 0) behind it.
        One decoder token per sentence and position over a key/value cache (csrc/kvq_generate.hip), no host read inside the loop;
        graph=True replays one captured step max_length - 1 times, graph=False launches it eagerly -- the same bits.
        top_k >= 1 / top_p < 1 (with temperature > 0) restrict the draw to the top_k most probable tokens and, of those, to the
        shortest prefix whose renormalised mass reaches top_p (HuggingFace's warpers, k first; ties by the lower id; DESIGN.md
        section 5k): the selection of the step is kvq_gen_select_filtered, the filters live in a device state beside the
        generation state, so one captured step serves every (top_k, top_p, temperature, seed).  want_scores: the log-probability
        of every chosen token under the distribution it was drawn from (at temperature 0: under the full softmax).  With neither,
        the call is the unfiltered one: the same launches, buffers and captured graph.
        Returns dict(ids [B, max_length], lengths [B], finished [B] bool [, logits [B, max_length - 1, V] f32: row t = what chose
        column t + 1] [, kept [B, max_length - 1] int: the size of the set row t drew from -- with a filter or want_scores]
        [, token_logprobs [B, max_length - 1] f32, scores [B] f64 = their sum over the positions that CHOSE a token (not the
        prompt, not the pads behind a finished sentence) -- with want_scores] [, indices]).  Meaningful for a model trained to predict the NEXT token (DECODER_NEXT_TOKEN); a model trained
        on the reference's unshifted loss reproduces its input token by construction."""
        self._latent_call("generate", refresh=False)
        self._check_generate(latents, max_length, prompt_ids, self.H, self.dtype, self.dev, int(self.dcfg.max_position_embeddings), temperature,
                             V=self.V, eos_id=eos_id, pad_id=pad_id, seed=seed)
        filtered = self._check_filters(top_k, top_p, temperature, want_scores, self.V)
        if quantize and not self.has_vq:
            raise KvqError("TrainEngine.generate: quantize=True, but the model has no quantiser")
        B, Se, _ = latents.shape
        L, P = int(max_length), prompt_ids.shape[1]
        self._seq_limit("generate", Se, L)
        self._latent_call("generate")               # (refuses first, then brings the flat buffers up to date: the first launches)
        res = {}
        if quantize:
            latents = self._quantized(latents, res)
        with torch.no_grad():
            g = self._gen_buffers(B, Se, L, want_logits, graph, filtered)
            self._gen_run(g, latents, prompt_ids, eos_id, pad_id, graph, float(temperature), int(seed) if temperature > 0 else 0,
                          nnops.gen_filter_words(int(top_k), float(top_p)) if filtered else None)
            res.update(ids=g["ids"][:B].clone(), lengths=g["lengths"][:B].long(), finished=g["finished"][:B] != 0)
            if want_logits:
                res["logits"] = g["step_logits"][:B, :L - 1].clone()
            if filtered:
                res["kept"] = g["kept"][:B, :L - 1].long()
            if want_scores:                         # row t chose column t + 1: a choice iff P <= t + 1 < lengths
                lp = g["logprob"][:B, :L - 1].clone()
                col = torch.arange(1, L, device=self.dev).unsqueeze(0)
                chose = (col >= P) & (col < res["lengths"].unsqueeze(1))
                res.update(token_logprobs=lp, scores=torch.where(chose, lp.double(), torch.zeros((), dtype=torch.float64, device=self.dev)).sum(dim=1))
        return res

    def _check_codes_call(self, who, indices, max_length, prompt_ids, kw, num_beams=None):
        """What generate_codes / beam_search_codes (with num_beams) refuse behind their own first refusals, in the order of the call
        they then make: every refusal in here comes before the lookup's launch.  -> the index rows [B, Se, G]."""
        self._latent_call(who, refresh=False)
        rows = self._code_rows(who, indices)
        ids_kw = dict(V=self.V, eos_id=kw.get("eos_id"), pad_id=kw.get("pad_id"))
        call = (rows.shape[0], max_length, prompt_ids, self.dev, int(self.dcfg.max_position_embeddings))
        if num_beams is None:
            self._check_generate_call(*call, kw.get("temperature", 0.0), seed=kw.get("seed", 0), **ids_kw)
            self._check_filters(kw.get("top_k", 0), kw.get("top_p", 1.0), kw.get("temperature", 0.0), kw.get("want_scores", False), self.V)
        else:
            self._check_beams(num_beams, kw.get("length_penalty", 0.0), self.V)
            self._check_generate_call(*call, 0.0, **ids_kw)
        self._seq_limit("generate" if num_beams is None else "beam_search", rows.shape[1], max_length)
        self._latent_call(who)
        return rows

    def generate_codes(self, indices, max_length, prompt_ids, **kw):
        """generate() of the codebook rows of `indices` [B, Se] / [B, Se, G] int64: as decode_codes is to decode."""
        if kw.get("quantize"):
            raise KvqError("TrainEngine.generate_codes: the latents are codebook rows already (quantize=True has nothing to do)")
        rows = self._check_codes_call("generate_codes", indices, max_length, prompt_ids, kw)
        return self.generate(self.codes_to_latents(rows), max_length, prompt_ids, **kw)

    # ------------------------------------------------------------------------------------------------------------
    # beam search: the same step on R = round_up(B W, 8) rows of slot space
    # ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_beams(num_beams, length_penalty, V):
        """What beam_search refuses beyond generate's refusals; needs no device."""
        if isinstance(num_beams, bool) or not isinstance(num_beams, int) or not 1 <= num_beams <= nnops.BEAM_MAX or num_beams > V:
            raise KvqError(f"TrainEngine.beam_search: num_beams must be an int in 1 .. {min(nnops.BEAM_MAX, V)}, got {num_beams!r}")
        if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float)) or not math.isfinite(length_penalty):
            raise KvqError(f"TrainEngine.beam_search: length_penalty must be a finite number, got {length_penalty!r}")

    def beam_search(self, latents, max_length, prompt_ids, num_beams, eos_id=None, pad_id=None, length_penalty=0.0, quantize=False,
                    want_trace=False, graph=True, **sampling):
        """The num_beams most probable continuations of the prompt under the free-running decoder of generate(): at every position
        the W = num_beams best of the live hypotheses' W V one-token extensions (by the sum of log-probabilities, ties to the lower
        beam, then the lower token) survive; a hypothesis that chooses eos_id is finished, keeps its score and keeps competing.
        The caches are never reordered: every row writes its own cache row once and reads its history through an ancestry table
        (kvq_beam_attn, kvq_beam_select).  No host read inside the loop; graph=True replays one captured step.
        The hypotheses are ranked once, at the end, by score / n^length_penalty (n = generated tokens, at least 1; f64, stable, -inf
        last); pruning inside the search is by the raw sum.  Returns dict(ids [B, L], lengths [B], finished [B]: the best
        hypothesis; beam_ids [B, W, L], beam_scores [B, W] f32 (raw sums), beam_lengths [B, W], beam_finished [B, W]: best first
        [, trace = dict(ids, parent, step_scores [B, W, L], logits [B, W, L - 1, V] f32), in slot space] [, indices]).
        top_k, top_p, temperature, seed, want_scores are refused by name: sampled beams are not supported."""
        self._refuse_sampling("beam_search", sampling)
        self._latent_call("beam_search", refresh=False)
        self._check_beams(num_beams, length_penalty, self.V)
        self._check_generate(latents, max_length, prompt_ids, self.H, self.dtype, self.dev, int(self.dcfg.max_position_embeddings), 0.0,
                             V=self.V, eos_id=eos_id, pad_id=pad_id)
        if quantize and not self.has_vq:
            raise KvqError("TrainEngine.beam_search: quantize=True, but the model has no quantiser")
        B, Se, _ = latents.shape
        L, P, W = int(max_length), prompt_ids.shape[1], int(num_beams)
        self._seq_limit("beam_search", Se, L)
        self._latent_call("beam_search")
        res = {}
        if quantize:
            latents = self._quantized(latents, res)
        with torch.no_grad():
            g = self._gen_buffers(B, Se, L, want_trace, graph, W=W)
            self._gen_run(g, latents, prompt_ids, eos_id, pad_id, graph)
            # ---- once per call: hypotheses out of slot space, the final ranking ----
            live = slice(0, B * W)
            hyp = nnops.beam_gather(g["state"], g["ids"], g["anc"], g["lengths"], out=g["hyp"])[live].view(B, W, L)
            scores, lengths = g["scores"][live].view(B, W), g["lengths"][live].view(B, W).long()
            n = (lengths - P).clamp(min=1).double()
            order = torch.sort(scores.double() / n.pow(float(length_penalty)), dim=1, descending=True, stable=True).indices
            res.update(beam_ids=hyp.gather(1, order.unsqueeze(-1).expand(B, W, L)), beam_scores=scores.gather(1, order),
                       beam_lengths=lengths.gather(1, order), beam_finished=(g["finished"][live].view(B, W) != 0).gather(1, order))
            res.update(ids=res["beam_ids"][:, 0].clone(), lengths=res["beam_lengths"][:, 0].clone(), finished=res["beam_finished"][:, 0].clone())
            if want_trace:
                res["trace"] = dict(ids=g["ids"][live].view(B, W, L).clone(), parent=g["parent"][live].view(B, W, L).clone(),
                                    step_scores=g["step_scores"][live].view(B, W, L).clone(),
                                    logits=g["step_logits"][live].view(B, W, L, self.V)[:, :, :L - 1].clone())
        return res

    def beam_search_codes(self, indices, max_length, prompt_ids, num_beams, **kw):
        """beam_search() of the codebook rows of `indices` [B, Se] / [B, Se, G] int64: as generate_codes is to generate."""
        if kw.get("quantize"):
            raise KvqError("TrainEngine.beam_search_codes: the latents are codebook rows already (quantize=True has nothing to do)")
        self._refuse_sampling("beam_search_codes", {k: v for k, v in kw.items() if k in self._SAMPLING_KEYS})
        rows = self._check_codes_call("beam_search_codes", indices, max_length, prompt_ids, kw, num_beams)
        return self.beam_search(self.codes_to_latents(rows), max_length, prompt_ids, num_beams, **kw)

    # ------------------------------------------------------------------------------------------------------------
    # free-running reconstruction metrics: encode -> generate from a start token -> compare with the input
    # ------------------------------------------------------------------------------------------------------------
    @classmethod
    def _check_reconstruct(cls, enc_ids, enc_mask, start_id, eos_id, target_ids, target_mask, max_length, slots, census, dev, V, sampling):
        """What reconstruct() refuses itself (generate / beam_search refuse the rest); needs no device.  -> (targets, their mask or
        None, max_length)."""
        cls._refuse_sampling("reconstruct", sampling, "an evaluation is deterministic and takes no {} (greedy generation, or beam "
                                                      "search with num_beams > 1)")
        if not torch.is_tensor(enc_ids) or enc_ids.dim() != 2 or enc_ids.dtype != torch.int64 or enc_ids.shape[0] < 1 or enc_ids.shape[1] < 1:
            raise KvqError("TrainEngine.reconstruct: enc_ids must be a non-empty int64 [B, S] tensor")
        if not torch.is_tensor(enc_mask) or enc_mask.shape != enc_ids.shape:
            raise KvqError("TrainEngine.reconstruct: enc_ids [B, S] needs an enc_mask of its shape")
        B, S = enc_ids.shape
        if isinstance(start_id, bool) or not isinstance(start_id, int) or not 0 <= start_id < V:
            raise KvqError(f"TrainEngine.reconstruct: start_id must be a token id (an int in [0, {V})), got {start_id!r}")
        if eos_id is not None and (isinstance(eos_id, bool) or not isinstance(eos_id, int) or not 0 <= eos_id < V):
            raise KvqError(f"TrainEngine.reconstruct: eos_id must be None or a token id (an int in [0, {V})), got {eos_id!r}")
        if max_length is None:
            max_length = S + 1
        if target_ids is None:
            if target_mask is not None:
                raise KvqError("TrainEngine.reconstruct: target_mask without target_ids (the encoder's mask goes with its ids)")
            target_ids, target_mask = enc_ids, enc_mask
        else:
            if not torch.is_tensor(target_ids) or target_ids.dim() != 2 or target_ids.dtype != torch.int64 or target_ids.shape[0] != B \
                    or target_ids.shape[1] < 1 or target_ids.device != dev:
                raise KvqError(f"TrainEngine.reconstruct: target_ids must be int64 [B, St] with B = {B} on {dev}")
            if eos_id is not None and target_mask is None:
                raise KvqError("TrainEngine.reconstruct: with an eos_id, target_ids needs a target_mask (its row sums are the "
                               "reference lengths)")
        if target_mask is not None and (not torch.is_tensor(target_mask) or target_mask.shape != target_ids.shape or target_mask.device != dev):
            raise KvqError(f"TrainEngine.reconstruct: target_mask must have target_ids' shape {tuple(target_ids.shape)} on {dev}")
        if slots is not None and census is None:
            raise KvqError("TrainEngine.reconstruct: slots without a census to add them to")
        if census is not None:
            from .census import ReconstructionCensus
            if not isinstance(census, ReconstructionCensus) or census.device != dev:
                raise KvqError(f"TrainEngine.reconstruct: census must be a kvq.census.ReconstructionCensus on {dev}")
            if slots is not None and (not torch.is_tensor(slots) or slots.dtype != torch.int32 or slots.dim() != 2 or slots.shape[0] != B
                                      or not 1 <= slots.shape[1] <= nnops.SEQ_TABLE_MAX_COLS or slots.device != dev):
                raise KvqError(f"TrainEngine.reconstruct: slots must be int32 [B, C] with B = {B}, C <= {nnops.SEQ_TABLE_MAX_COLS} on {dev} "
                               f"(ReconstructionCensus.slots_of)")
        return target_ids, target_mask, max_length

    def reconstruct(self, enc_ids, enc_mask, start_id, eos_id=None, target_ids=None, target_mask=None, max_length=None, num_beams=1,
                    length_penalty=0.0, slots=None, census=None, want_ids=False, graph=True, **sampling):
        """Does the latent alone give the sentence back?  encode() (the quantiser in evaluation mode; the latents are z_q, else z),
        generate() greedily from a column of start_id up to max_length (default S + 1) -- or the best hypothesis of beam_search()
        with num_beams > 1 --, then kvq_seq_compare of what was written behind the start token against target_ids (default:
        enc_ids) and, with a census (kvq.census.ReconstructionCensus), kvq_seq_compare_accumulate into its table at the rows
        `slots` [B, C] int32 (default: row 0 for every sentence).
        Lengths: with an eos_id the reference is the first sum(target_mask[b]) tokens (default mask: enc_mask) and the hypothesis
        ends with its end token; without one both sides are every column, pads included (max_length - 1 generated tokens against
        all of target_ids: the reference project's accuracy convention).
        Returns device tensors dict(dist, hits, hyp_len, ref_len [B] int32, exact [B] bool, n_bad int64 [1]: the sentences whose
        lengths did not fit, dist = -1 there [, ids [B, max_length], lengths [B] with want_ids]).  No host read beyond
        generate()'s prompt-range check.  Refuses what encode / generate / beam_search refuse, and every sampling argument."""
        self._latent_call("reconstruct", refresh=False)
        tgt, tmask, L = self._check_reconstruct(enc_ids, enc_mask, start_id, eos_id, target_ids, target_mask, max_length, slots, census,
                                                self.dev, self.V, sampling)
        if num_beams != 1:
            self._check_beams(num_beams, length_penalty, self.V)
        B, S = enc_ids.shape
        prompt = torch.full((B, 1), int(start_id), dtype=torch.int64, device=self.dev)
        self._check_generate_call(B, L, prompt, self.dev, int(self.dcfg.max_position_embeddings), 0.0, eos_id=eos_id)
        self._seq_limit("reconstruct", S, L, tgt.shape[1])
        enc = self.encode(enc_ids, enc_mask)
        lat = (enc["z_q"] if self.has_vq else enc["z"]).reshape(B, S, self.H)
        if num_beams == 1:
            gen = self.generate(lat, L, prompt, eos_id=eos_id, graph=graph)
        else:
            gen = self.beam_search(lat, L, prompt, num_beams, eos_id=eos_id, length_penalty=length_penalty, graph=graph)
        with torch.no_grad():
            ids = gen["ids"]
            St = tgt.shape[1]
            ref_len = torch.full((B,), St, dtype=torch.int32, device=self.dev) if eos_id is None else tmask.sum(dim=1).to(torch.int32)
            n_bad = torch.zeros(1, dtype=torch.int64, device=self.dev)
            per, _ = nnops.seq_compare(ids, gen["lengths"].to(torch.int32), tgt, ref_len, hyp_skip=1, Lmax=max(L - 1, St), n_bad=n_bad)
            if census is not None:
                if slots is None:
                    slots = torch.zeros((B, 1), dtype=torch.int32, device=self.dev)
                nnops.seq_compare_accumulate(per, slots.contiguous(), census.table)
                census.n_bad += n_bad
            res = dict(dist=per[:, 0], hits=per[:, 1], hyp_len=per[:, 2], ref_len=per[:, 3], exact=per[:, 0] == 0, n_bad=n_bad)
            if want_ids:
                res.update(ids=ids, lengths=gen["lengths"])
        return res

    def traverse_codes(self, enc_ids, enc_mask, sentence, position, dec_ids=None, dec_mask=None, factor=0, free_running=False,
                       max_length=None, start_id=None, num_beams=1, length_penalty=0.0, temperature=0.0, seed=0, top_k=0, top_p=1.0,
                       want_scores=False):
        """Every code at one place of one sentence: encodes the batch, takes sentence `sentence`'s own index rows [Se, G], builds the
        K variants that differ from them only at (position, factor) -- variant k carries code k there -- and decodes them with
        that sentence's decoder ids (default: its encoder ids), at most 256 variants per launch sequence.
        free_running=True: the variants are GENERATED (generate_codes, greedy) from start_id (default: the first decoder id of the
        sentence) up to max_length (default: the decoder ids' length) instead of decoded against the sentence's own ids;
        num_beams > 1: each variant's row is the best hypothesis of beam_search_codes (length_penalty: its final ranking);
        temperature, seed, top_k, top_p (num_beams == 1): the variants are SAMPLED as generate() samples; want_scores: scores [K],
        the sum of the chosen tokens' log-probabilities of every variant (generate's).
        Returns dict(recon_ids [K, Sd], own_code (int), changed [K, Sd] bool: tokens that differ from the own code's row
        [, beam_ids [K, W, Sd], beam_scores [K, W]: every variant's hypotheses, best first, with num_beams = W > 1])."""
        self._latent_call("traverse_codes", refresh=False)
        sampling = dict(temperature=temperature, seed=seed, top_k=top_k, top_p=top_p, want_scores=want_scores)
        if sampling != self._SAMPLING_DEFAULTS:
            if not free_running:
                raise KvqError("TrainEngine.traverse_codes: temperature, seed, top_k, top_p and want_scores apply with free_running=True")
            if num_beams != 1:
                self._refuse_sampling("traverse_codes", {k: v for k, v in sampling.items() if v != self._SAMPLING_DEFAULTS[k]})
            self._check_filters(top_k, top_p, temperature, want_scores, self.V)
        self._latent_call("traverse_codes")
        if self.vq_kind not in ("VectorQuantizer", "MultiVectorQuantizer"):
            raise KvqError(f"TrainEngine.traverse_codes: needs a VectorQuantizer or MultiVectorQuantizer codebook (this model has "
                           f"{self.vq_kind or 'no quantiser'})")
        d_ids = enc_ids if dec_ids is None else dec_ids
        d_mask = enc_mask if dec_mask is None else dec_mask
        B, Se = enc_ids.shape
        if not (0 <= int(sentence) < B and 0 <= int(position) < Se and 0 <= int(factor) < self.G):
            raise KvqError(f"TrainEngine.traverse_codes: (sentence, position, factor) = ({sentence}, {position}, {factor}) outside "
                           f"({B}, {Se}, {self.G})")
        if d_ids.shape[0] != B or d_mask.shape != d_ids.shape:
            raise KvqError("TrainEngine.traverse_codes: dec_ids needs the encoder's batch size and a dec_mask of its shape")
        own = self.encode(enc_ids, enc_mask)["indices"].reshape(B, Se, self.G)[int(sentence)]
        own_code = int(own[int(position), int(factor)].item())
        K = self.K
        rows = own.unsqueeze(0).repeat(K, 1, 1)
        rows[:, int(position), int(factor)] = torch.arange(K, dtype=torch.int64, device=self.dev)
        recon, beams, scores = [], [], []
        for k0 in range(0, K, self._TRAVERSE_CHUNK):
            n = min(self._TRAVERSE_CHUNK, K - k0)
            if free_running:
                start = int(d_ids[int(sentence), 0].item()) if start_id is None else int(start_id)
                gen_args = (rows[k0:k0 + n], int(d_ids.shape[1] if max_length is None else max_length),
                            torch.full((n, 1), start, dtype=torch.int64, device=self.dev))
                if num_beams == 1:
                    out = self.generate_codes(*gen_args, **sampling)
                    if want_scores:
                        scores.append(out["scores"])
                else:
                    out = self.beam_search_codes(*gen_args, num_beams, length_penalty=length_penalty)
                    beams.append((out["beam_ids"], out["beam_scores"]))
                recon.append(out["ids"])
                continue
            out = self.decode_codes(rows[k0:k0 + n], d_ids[int(sentence)].unsqueeze(0).expand(n, -1).contiguous(),
                                    d_mask[int(sentence)].unsqueeze(0).expand(n, -1).contiguous())
            recon.append(out["recon_ids"])
        recon = torch.cat(recon)
        res = dict(recon_ids=recon, own_code=own_code, changed=recon != recon[own_code].unsqueeze(0))
        if beams:
            res.update(beam_ids=torch.cat([b[0] for b in beams]), beam_scores=torch.cat([b[1] for b in beams]))
        if scores:
            res["scores"] = torch.cat(scores)
        return res
