"""Device-resident census tables: the word x code census of the quantiser's indices (host side of `kvq_code_census`,
include/kvq.h), the attention-map census (`AttentionCensus`, host side of `kvq_attn_probs`), the group means of encoder outputs
(`LatentCensus`, host side of `kvq_latent_group_sum` / `kvq_latent_shift`) and, at the end of the file, the free-running
reconstruction metrics summed per generative-factor value (`ReconstructionCensus`, host side of `kvq_seq_compare_accumulate`).

Boundary mirrored: the bookkeeping of analyses/unsupervised_vq_disentanglement/unsupervised_vq_disentanglement.py:156-235.
The reference walks sentence -> word -> token in Python, tokenising every word of every sentence again to learn how many
tokens it has (:174), and appends to Python lists; here

* `WordSpanIndex` turns sentences into ONE int32 per token position (-1 = no word, else (slot << 1) | first-token flag), with
  the per-word token count memoised (each distinct word is tokenised once);
* `CodeCensus` keeps counts[G][W][K] for all tokens and for first tokens on the device, one kernel per batch, no host sync;
* `CodeCensus.results()` reads the tables back once and derives what the reference writes to its three files.
"""
from __future__ import annotations

from typing import Dict, Iterable, List, Sequence

import torch

from ._ffi import KvqError, check, lib, require_gpu, stream_ptr


class WordSpanIndex:
    """Distinct words (as written: the reference compares `word in WORDS_OF_INTEREST` on the raw string, :185) -> slots in
    first-seen order; sentences -> the per-position int32 the kernel reads."""

    def __init__(self, tokenizer):
        self.tokenizer = tokenizer
        self.slot_of: Dict[str, int] = {}
        self.words: List[str] = []
        self._ntok: Dict[str, int] = {}

    def _n_tokens(self, word: str) -> int:
        n = self._ntok.get(word)
        if n is None:                         # (:174) tokenizer(word, padding=False, add_special_tokens=False).input_ids.flatten()
            ids = self.tokenizer(word, return_tensors="pt", padding=False, add_special_tokens=False).input_ids
            n = int(ids.numel())
            self._ntok[word] = n
        return n

    def slot(self, word: str) -> int:
        s = self.slot_of.get(word)
        if s is None:
            s = len(self.words)
            self.slot_of[word] = s
            self.words.append(word)
        return s

    def slot_first(self, sentences: Sequence[str], width: int) -> torch.Tensor:
        """[len(sentences), width] int32 (host): the words of a sentence laid over its token positions in order (:170-178).
        A sentence whose words need more than `width` positions is an error (the reference would index past the row)."""
        out = torch.full((len(sentences), width), -1, dtype=torch.int32)
        for r, s in enumerate(sentences):
            pos = 0
            for word in s.split(" "):
                n = self._n_tokens(word)
                if n == 0:
                    continue
                if pos + n > width:
                    raise KvqError(f"WordSpanIndex: sentence {s!r} needs more than {width} token positions")
                sl = self.slot(word) << 1
                out[r, pos] = sl | 1
                if n > 1:
                    out[r, pos + 1:pos + n] = sl
                pos += n
        return out


class CodeCensus:
    """Device tables counts_all / counts_first [G][W][K] uint32 (W = capacity in distinct words), accumulated over batches."""

    def __init__(self, n_codes: int, capacity_words: int, n_factors: int = 1, device=None):
        if n_codes < 1 or capacity_words < 1 or n_factors < 1:
            raise KvqError("CodeCensus: n_codes, capacity_words, n_factors >= 1")
        self.K, self.W, self.G = int(n_codes), int(capacity_words), int(n_factors)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise KvqError("CodeCensus: the tables live on the GPU (no CPU path)")
        # uint32 cells kept in int32 storage (torch has no uint32 arithmetic; the bits are read back as unsigned)
        self._all = torch.zeros((self.G, self.W, self.K), dtype=torch.int32, device=self.device)
        self._first = torch.zeros_like(self._all)
        self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.tokens = 0

    def add(self, slot_first: torch.Tensor, indices: torch.Tensor) -> None:
        """slot_first [B, S] int32, indices [B, S, 1] / [B, S] / [B, S, G] int64 (min_encoding_indices), both on the device."""
        require_gpu(slot_first, indices)
        if slot_first.dtype != torch.int32 or indices.dtype != torch.int64:
            raise KvqError("CodeCensus.add: slot_first int32, indices int64")
        n = slot_first.numel()
        if indices.numel() != n * self.G:
            raise KvqError(f"CodeCensus.add: {indices.numel()} indices for {n} positions x {self.G} factors")
        sf, ix = slot_first.contiguous(), indices.contiguous()
        check(lib().kvq_code_census(sf.data_ptr(), ix.data_ptr(), n, self.G, self.K, self.W, self._all.data_ptr(),
                                    self._first.data_ptr(), self._bad.data_ptr(), stream_ptr()), "kvq_code_census")
        self.tokens += n

    def tables(self):
        """(counts_all, counts_first) as int64 [G, W, K] on the host, and the number of skipped positions."""
        u = lambda t: t.cpu().to(torch.int64) & 0xFFFFFFFF
        return u(self._all), u(self._first), int(self._bad.item())

    def results(self, words: Sequence[str], words_of_interest: Iterable[str], factor: int = 0) -> dict:
        """What the reference writes (:208-235), for one factor's codebook:
        populated          -- set of codes that received a token                                   (seen_v_is)
        histograms[word]   -- {code: times the word's FIRST token took that code} for words of interest, every code 0..K-1 present
        words_of_code[k]   -- the distinct words with a token on code k (sorted; the reference's list(set(...)) has no order)"""
        call, cfirst, bad = self.tables()
        if bad:
            raise KvqError(f"CodeCensus: {bad} positions had a slot beyond the capacity or a code outside [0, {self.K})")
        if len(words) > self.W:
            raise KvqError("CodeCensus.results: more words than table rows")
        a, f = call[factor, :len(words)], cfirst[factor, :len(words)]
        slot_of = {w: i for i, w in enumerate(words)}
        populated = set(torch.nonzero(a.sum(0)).flatten().tolist())
        histograms = {}
        for w in words_of_interest:
            row = f[slot_of[w]].tolist() if w in slot_of else [0] * self.K
            histograms[w] = {k: int(row[k]) for k in range(self.K)}
        words_of_code = {k: sorted(words[i] for i in torch.nonzero(a[:, k]).flatten().tolist()) for k in range(self.K)}
        return {"populated": populated, "histograms": histograms, "words_of_code": words_of_code}


ATTENTION_FAMILIES = ("enc_self", "dec_self", "cross")


class AttentionCensus:
    """Mean attention maps over everything seen, one f64 table [L, nh, queries, keys] per family on the device -- the content of
    analyses/cross_attention/extract_model_cross_attention.py's `*_mean_across_batch_size.pth` (:103-108), without its host
    copies of every batch (:85-86: "had to limit to 69 batches in order to avoid memory crashes").
    Sq / Sk: the decoder's / the encoder's padded length.  "dec_self" is [L, nh, Sq, Sq], "cross" [L, nh, Sq, Sk], "enc_self"
    [L, nh, Sk, Sk].  TrainEngine.attention_maps(..., census=self) adds each batch's sum over sentences (kvq_attn_probs: f64,
    no atomics, the same bits on every run) and the sentence count; results() reads the tables back once."""

    def __init__(self, n_layers: int, n_heads: int, Sq: int, Sk: int, families=("dec_self", "cross"), device=None):
        if n_layers < 1 or n_heads < 1 or Sq < 1 or Sk < 1:
            raise KvqError("AttentionCensus: n_layers, n_heads, Sq, Sk >= 1")
        if max(Sq, Sk) > 128:
            raise KvqError("AttentionCensus: the attention kernels end at 128 tokens")
        families = tuple(families)
        if not families or any(f not in ATTENTION_FAMILIES for f in families) or len(set(families)) != len(families):
            raise KvqError(f"AttentionCensus: families must be distinct names out of {ATTENTION_FAMILIES}, got {families}")
        self.L, self.nh, self.Sq, self.Sk, self.families = int(n_layers), int(n_heads), int(Sq), int(Sk), families
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise KvqError("AttentionCensus: the tables live on the GPU (no CPU path)")
        dims = {"enc_self": (self.Sk, self.Sk), "dec_self": (self.Sq, self.Sq), "cross": (self.Sq, self.Sk)}
        self.tables = {f: torch.zeros((self.L, self.nh) + dims[f], dtype=torch.float64, device=self.device) for f in families}
        self.count = 0                        # sentences seen

    def require(self, family, n_layers, n_heads, n_queries, n_keys, device) -> None:
        """Raises unless the table of `family` is [n_layers, n_heads, n_queries, n_keys] on `device`."""
        t = self.tables.get(family)
        want = (n_layers, n_heads, n_queries, n_keys)
        if t is None or tuple(t.shape) != want or t.device != torch.device(device):
            raise KvqError(f"AttentionCensus: the {family!r} table is {None if t is None else tuple(t.shape)} on {self.device}; "
                           f"this model and batch need {want} on {device}")

    def results(self) -> Dict[str, torch.Tensor]:
        """{family: float32 [L, nh, queries, keys]} on the host: table / sentences seen."""
        if self.count < 1:
            raise KvqError("AttentionCensus.results: no sentence was added")
        return {f: (t.cpu() / self.count).to(torch.float32) for f, t in self.tables.items()}


class LatentCensus:
    """Per-group sums of encoder outputs, one f64 table [n_groups, S, H] and one int64 count per group on the device -- the means
    analyses/latent_arithmetics/latent_arithmetics_Bagon.py:97-131 takes over host copies of every encoder output ("300 sentences
    per group"), with no limit on batches or sentences.  add() is one kvq_latent_group_sum per batch (f64, no float atomics, the
    same bits on every run) and never synchronises; results() reads tables, counts and the bad-label word back once.
    direction(g1, g0) = mean(g1) - mean(g0) on the host; shift() adds alpha times that difference to latents on the device
    (kvq_latent_shift), which is what the reference feeds the decoder as encoder_hidden_states."""

    def __init__(self, n_groups: int, S: int, H: int, device=None):
        if n_groups < 1 or S < 1 or H < 1:
            raise KvqError("LatentCensus: n_groups, S, H >= 1")
        self.G, self.S, self.H = int(n_groups), int(S), int(H)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise KvqError("LatentCensus: the tables live on the GPU (no CPU path)")
        self.table = torch.zeros((self.G, self.S, self.H), dtype=torch.float64, device=self.device)
        self.count = torch.zeros(self.G, dtype=torch.int64, device=self.device)
        self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._host = None                     # results() of the tables as they are now
        self.sentences = 0                    # handed to add(), skipped ones included

    def _check_latents(self, latents, what):
        require_gpu(latents)
        if latents.dim() != 3 or tuple(latents.shape[1:]) != (self.S, self.H):
            raise KvqError(f"LatentCensus.{what}: latents must be [B, {self.S}, {self.H}], got {tuple(latents.shape)}")
        if latents.dtype not in (torch.float32, torch.bfloat16):
            raise KvqError(f"LatentCensus.{what}: latents must be float32 or bfloat16, got {latents.dtype}")
        if latents.device != self.device:
            raise KvqError(f"LatentCensus.{what}: latents on {latents.device}, tables on {self.device}")

    def add(self, latents: torch.Tensor, group) -> None:
        """latents [B, S, H] (f32 / bf16, on the device); group: one label for the whole batch, or [B] integer labels (a tensor
        on either side, or a sequence): -1 = leave the sentence out, 0 .. n_groups-1 = its group.  A label outside that range is
        found by results()."""
        from . import nnops
        self._check_latents(latents, "add")
        B = latents.shape[0]
        if isinstance(group, int):
            group = torch.full((B,), group, dtype=torch.int32, device=self.device)
        elif not torch.is_tensor(group):
            group = torch.tensor(list(group), dtype=torch.int32)
        if group.dim() != 1 or group.numel() != B or group.is_floating_point() or group.dtype == torch.bool:
            raise KvqError(f"LatentCensus.add: group must be an int or {B} integer labels")
        group = group.to(device=self.device, dtype=torch.int32).contiguous()
        if B == 0:
            return
        nnops.latent_group_sum(latents, group, self.table, self.count, self._bad)
        self._host = None
        self.sentences += B

    def results(self) -> dict:
        """dict(mean = float64 [n_groups, S, H] (zeros for an empty group), count = int64 [n_groups]) on the host."""
        if self._host is None:
            n = self.G * self.S * self.H
            # one read-back: the table, then counts and the bad-label word as their exact f64 values (counts stay below 2^53)
            flat = torch.cat([self.table.reshape(-1), self.count.to(torch.float64), self._bad.to(torch.float64)]).cpu()
            bad = int(flat[n + self.G].item()) & 0xFFFFFFFF
            if bad:
                raise KvqError(f"LatentCensus: {bad} sentences carried a group label outside [-1, {self.G})")
            count = flat[n:n + self.G].to(torch.int64)
            mean = flat[:n].view(self.G, self.S, self.H) / count.clamp(min=1).to(torch.float64).view(-1, 1, 1)
            self._host = dict(mean=mean, count=count)
        return self._host

    def _require_filled(self, what, *groups):
        res = self.results()
        for g in groups:
            if not 0 <= int(g) < self.G:
                raise KvqError(f"LatentCensus.{what}: group {g} outside [0, {self.G})")
            if int(res["count"][int(g)]) == 0:
                raise KvqError(f"LatentCensus.{what}: group {g} is empty")
        return res

    def direction(self, g1: int, g0: int) -> torch.Tensor:
        """mean(g1) - mean(g0), float64 [S, H] on the host."""
        res = self._require_filled("direction", g1, g0)
        return res["mean"][int(g1)] - res["mean"][int(g0)]

    def shift(self, latents: torch.Tensor, g1: int, g0: int, alpha: float = 1.0, sel=None, out=None) -> torch.Tensor:
        """latents + alpha * (mean(g1) - mean(g0)) at the positions with sel[b, s] != 0 (sel: [B, S] bool / int8 on the device, None
        = every position), the unchanged bits elsewhere; f64 arithmetic rounded to f32, then to the latents' dtype.  out=latents
        shifts in place.  An empty group is refused (the counts are known from results())."""
        from . import nnops
        self._check_latents(latents, "shift")
        self._require_filled("shift", g1, g0)
        if sel is not None:
            require_gpu(sel)
            if tuple(sel.shape) != tuple(latents.shape[:2]):
                raise KvqError(f"LatentCensus.shift: sel must be [B, S] = {tuple(latents.shape[:2])}, got {tuple(sel.shape)}")
            sel = (sel != 0).to(torch.int8).contiguous()
        return nnops.latent_shift(latents, self.table, self.count, int(g1), int(g0), float(alpha), sel=sel, out=out)


class ReconstructionCensus:
    """Free-running reconstruction metrics summed over everything seen: one int64 table [R, 6] of
    (sentences, exact matches, edit distance, positional hits, hypothesis tokens, reference tokens) and the count of sentences
    whose lengths did not fit, on the device.  Row 0 is "all sentences"; behind it one row per (factor, value) of the dataset's
    generative factors, laid out by the prefix sums of `cardinalities` (rows()).  TrainEngine.reconstruct(..., slots=
    census.slots_of(labels), census=census) adds a batch (kvq_seq_compare_accumulate: integer sums, no host read);
    result() reads the table back once.  The table may live on the CPU for slots_of / result (tests, merging saved tables);
    reconstruct needs it on the engine's device."""
    COLUMNS = ("sentences", "exact", "dist", "hits", "hyp_tokens", "ref_tokens")

    def __init__(self, cardinalities=None, device=None):
        cards = [] if cardinalities is None else list(cardinalities)
        if any(isinstance(c, bool) or not isinstance(c, int) or c < 1 for c in cards):
            raise KvqError(f"ReconstructionCensus: cardinalities must be ints >= 1, got {cardinalities!r}")
        self.cardinalities = cards
        self.offsets = [1 + sum(cards[:f]) for f in range(len(cards))]        # first row of factor f
        self.R = 1 + sum(cards)
        if self.R > 4096 or len(cards) + 1 > 16:
            raise KvqError(f"ReconstructionCensus: {self.R} rows / {len(cards)} factors above the kernel's limits (4096 rows, 15 factors)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.table = torch.zeros((self.R, 6), dtype=torch.int64, device=self.device)
        self.n_bad = torch.zeros(1, dtype=torch.int64, device=self.device)

    def reset(self) -> None:
        self.table.zero_()
        self.n_bad.zero_()

    def rows(self):
        """[(factor, value)] per table row; row 0 is (None, None)."""
        return [(None, None)] + [(f, v) for f, c in enumerate(self.cardinalities) for v in range(c)]

    def slots_of(self, labels: torch.Tensor) -> torch.Tensor:
        """labels [B, F] integers (F = number of factors) -> int32 [B, F + 1] on the census' device: column 0 is row 0 for every
        sentence, column f + 1 the row of (f, labels[b, f]); a label outside its factor's range maps to -1 (skipped).  No host
        read."""
        F = len(self.cardinalities)
        if not torch.is_tensor(labels) or labels.dim() != 2 or labels.shape[1] != F or labels.is_floating_point() or labels.dtype == torch.bool:
            raise KvqError(f"ReconstructionCensus.slots_of: labels must be an integer [B, {F}] tensor")
        lab = labels.to(device=self.device, dtype=torch.int64)
        out = torch.zeros((lab.shape[0], F + 1), dtype=torch.int32, device=self.device)
        if F:
            card = torch.tensor(self.cardinalities, dtype=torch.int64, device=self.device)
            off = torch.tensor(self.offsets, dtype=torch.int64, device=self.device)
            ok = (lab >= 0) & (lab < card)
            out[:, 1:] = torch.where(ok, lab + off, torch.full_like(lab, -1)).to(torch.int32)
        return out

    def result(self) -> dict:
        """One read-back.  dict(sentences int64 [R], exact, token_acc, edit_rate, len_ratio float64 [R], n_bad int, rows):
        exact = exact matches / sentences, token_acc = hits / reference tokens, edit_rate = distance / reference tokens,
        len_ratio = hypothesis tokens / reference tokens; nan for a row without sentences."""
        flat = torch.cat([self.table.reshape(-1), self.n_bad.reshape(-1)]).cpu()
        t = flat[:-1].view(self.R, 6)
        n, ref = t[:, 0], t[:, 5].to(torch.float64)
        nan = torch.full((self.R,), float("nan"), dtype=torch.float64)
        some = n > 0
        per_ref = lambda c: torch.where(some, t[:, c].to(torch.float64) / ref, nan)
        return dict(sentences=n.clone(), exact=torch.where(some, t[:, 1].to(torch.float64) / n.to(torch.float64), nan),
                    token_acc=per_ref(3), edit_rate=per_ref(2), len_ratio=per_ref(4), n_bad=int(flat[-1]), rows=self.rows())
