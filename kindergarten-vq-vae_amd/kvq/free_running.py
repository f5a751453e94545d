"""Free-running evaluation in the trainers (FREE_RUNNING_EVAL): what both entry points and both Trainer
modules share -- the configuration refusals, the per-stage bookkeeping around TrainEngine.reconstruct and a
kvq.census.ReconstructionCensus, the extra columns of decoded_sentences.* and reconstruction_by_factor.md.

Off by default: with the option off none of this is constructed and no stage launches, reads or logs anything it did not before.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

FR_KEYS = ("fr_exact", "fr_token_acc", "fr_edit_rate")


def check_free_running_config(free_running_eval, free_running_eval_val, beams, decoder_next_token, use_engine, world=1) -> None:
    """What main() refuses before any training: a ValueError naming the constant."""
    for name, v in (("FREE_RUNNING_EVAL", free_running_eval), ("FREE_RUNNING_EVAL_VAL", free_running_eval_val)):
        if not isinstance(v, bool):
            raise ValueError(f"{name} (KVQ_{name}) must be True or False, got {v!r}")
    if isinstance(beams, bool) or not isinstance(beams, int) or not 1 <= beams <= 8:
        raise ValueError(f"FREE_RUNNING_EVAL_BEAMS (KVQ_FREE_RUNNING_EVAL_BEAMS) must be an integer in 1 .. 8, got {beams!r}")
    if free_running_eval_val and not free_running_eval:
        raise ValueError("FREE_RUNNING_EVAL_VAL adds validation to FREE_RUNNING_EVAL: set FREE_RUNNING_EVAL as well")
    if not free_running_eval:
        return
    if not decoder_next_token:
        raise ValueError("FREE_RUNNING_EVAL needs DECODER_NEXT_TOKEN: a decoder trained on the unshifted loss copies its input token, "
                         "and what it generates from a start token says nothing about the latent")
    if not use_engine:
        raise ValueError("FREE_RUNNING_EVAL needs the engine (USE_ENGINE and a model shape it supports): generation runs on its "
                         "key/value-cache decoder")
    if world != 1:
        raise ValueError(f"FREE_RUNNING_EVAL needs a single process (TrainEngine.reconstruct refuses a process group), got {world}")


def label_cardinalities(labels) -> Optional[list]:
    """[max label + 1 per factor] of a dataset's latent_classes_labels [M, F] (None without labels): one host pass, at start-up."""
    if labels is None or len(labels) == 0:
        return None
    return [int(v) + 1 for v in labels.max(dim=0).values.tolist()]


class FreeRunningEval:
    """One per run.  runs(stage) says whether a stage evaluates; begin() clears the census, batch() adds a batch (one
    TrainEngine.reconstruct, no host read of its own), finish() reads the census once and returns the stage's three numbers."""

    def __init__(self, engine, start_id: int, eos_id: Optional[int] = None, num_beams: int = 1, validation: bool = False,
                 cardinalities: Optional[Sequence[int]] = None):
        from .census import ReconstructionCensus
        self.engine, self.start_id, self.eos_id, self.num_beams, self.validation = engine, int(start_id), eos_id, int(num_beams), bool(validation)
        self.census = ReconstructionCensus(cardinalities, device=engine.dev)
        self.last = None                      # result() of the last finished stage

    def runs(self, stage: str) -> bool:
        return stage == "test" or (stage == "val" and self.validation)

    def begin(self) -> None:
        self.census.reset()

    def batch(self, enc_ids, enc_mask, target_ids=None, target_mask=None, labels=None, want_ids=False) -> dict:
        slots = None
        if labels is not None and self.census.cardinalities:
            slots = self.census.slots_of(labels[:, :len(self.census.cardinalities)])
        return self.engine.reconstruct(enc_ids, enc_mask, self.start_id, eos_id=self.eos_id, target_ids=target_ids, target_mask=target_mask,
                                       num_beams=self.num_beams, slots=slots, census=self.census, want_ids=want_ids)

    def finish(self) -> dict:
        self.last = self.census.result()
        return {k: float(self.last[src][0]) for k, src in zip(FR_KEYS, ("exact", "token_acc", "edit_rate"))}

    def write_report(self, path: str, stage: str, factor_names: Optional[Sequence[str]] = None) -> None:
        """reconstruction_by_factor.md: the last finished stage, one line per factor value behind the line of all sentences."""
        res = self.last
        if res is None:
            return
        cell = lambda v: "nan" if math.isnan(v) else f"{v:.6f}"
        rows = ["# Free-running reconstruction by generative factor", "",
                f"Stage `{stage}`: " + (f"the best of {self.num_beams} beams" if self.num_beams > 1 else "greedy generation") + " from the latent"
                + f"; sentences whose lengths did not fit: {res['n_bad']}.", "",
                "| factor | value | sentences | exact | token_acc | edit_rate | len_ratio |", "|---|---|---|---|---|---|---|"]
        for r, (f, v) in enumerate(res["rows"]):
            name = "all" if f is None else (factor_names[f] if factor_names is not None and f < len(factor_names) else f"factor_{f}")
            rows.append(f"| {name} | {'' if v is None else v} | {int(res['sentences'][r])} | " +
                        " | ".join(cell(float(res[k][r])) for k in ("exact", "token_acc", "edit_rate", "len_ratio")) + " |")
        with open(path, "w") as fp:
            fp.write("\n".join(rows) + "\n")


def decoded_columns(rec: dict, tokenizer) -> list:
    """Per sentence of a batch: dict(free_running_sentence, free_running_edit_distance, free_running_exact) from a
    reconstruct(want_ids=True) result -- the generated tokens behind the start token up to the sentence's length."""
    ids, lengths = rec["ids"].cpu(), rec["lengths"].cpu().tolist()
    dist, exact = rec["dist"].cpu().tolist(), rec["exact"].cpu().tolist()
    rows = [ids[b, 1:max(int(n), 1)].tolist() for b, n in enumerate(lengths)]
    try:
        text = tokenizer.batch_decode(sequences=rows, skip_special_tokens=True)
    except TypeError:                                               # the offline word tokenizer has no such switch
        text = tokenizer.batch_decode(sequences=rows)
    return [dict(free_running_sentence=t, free_running_edit_distance=int(d), free_running_exact=bool(x)) for t, d, x in zip(text, dist, exact)]
