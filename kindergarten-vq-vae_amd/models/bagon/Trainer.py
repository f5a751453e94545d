"""step / train / test of the plain Bagon run -- counterpart of models/bagon/Trainer.py:65-510.

Kept from the reference: function names and keyword lists (two tokenizers with their own add-special-tokens flag and padded
length, the four perturbation percentages, vocabulary sizes), the per-step stats dict and its keys (`loss_recon_step`,
`loss_full_step`, `metric_acc_step_per_batch`, `metric_acc_step_per_sentence`, `padding_tokens_pct_step` = -69), the 5-tuple
`step()` returns (stats, encoder ids, decoder ids, recon ids, latent class labels), running / best bookkeeping and its keys,
`decode_sentences` rows (with the per-sentence accuracy and the explicit latent labels), checkpoint names
(`bagon_ckpt_{loss_recon,metric_acc}_{stage}_best.pth`) and keys.  As in the reference (Trainer.py:94,103-106) the loss and the
accuracy score the logits against the decoder's input ids AFTER their perturbation.

Two execution paths for one step:
  * engine (default, `engine=` a kvq.engine.TrainEngine): forward, loss, backward, gradient exchange, Adam and the per-step
    scheduler tick are the engine's hand-written HIP schedule (kvq/engine.py), replayed from hipGraphs; the encoder and decoder
    sides keep their own ids (the decoder's feed the decoder's embedding table, the loss target and its word-embedding gradient);
  * autograd (`engine=None`): kvq/bert.py under torch autograd + the fused loss kernel + torch.optim.Adam -- the checker.

Deviations from reference quirks, documented in DESIGN.md §6: running means are weighted by the true batch size (the reference
weights by len(batch-dict) == 3, which cancels out in the means), stats stay on the device until the end of the epoch, batches
are consumed lazily instead of `list(dl_train)`, the "val" checkpoint is decided by the VAL best flags (the reference passes the
TRAIN flags, Trainer.py:437), the progress display is optional (`prg=None`)."""
from __future__ import annotations

import time as _time
from itertools import islice

import numpy as np
import torch
from torch import Tensor, no_grad, save

from common.consts import *  # noqa: F401,F403
from common.tensor_utils import replace_pct_rand_values
from kvq.runlog import (drop_open_accumulation, grad_guard_epoch_record, grad_norm_note, optimizer_step_note, optimizer_steps_epoch,
                        weight_ema_epoch_record, weight_ema_scope, lr_epoch_record, param_groups_line)
from kvq.free_running import FR_KEYS, decoded_columns
from kvq.train_state import check_every, restore_trainer, save_train_state, trainer_state


def _tokenize(batch, tokenizer, add_special_tokens, max_length, device, side):
    """Trainer.py:78-84 / :87-93.  Batches that already carry ids (pre-tokenised cache) skip the tokenizer."""
    key = f"input_ids_{side}" if f"input_ids_{side}" in batch else "input_ids"
    if key in batch:
        ids, mask = batch[key], batch[key.replace("input_ids", "attention_mask")]
    else:
        tok = tokenizer(batch["sentence"], return_tensors="pt", padding="max_length", max_length=max_length,
                        add_special_tokens=add_special_tokens)
        ids, mask = tok.input_ids, tok.attention_mask
    return ids.to(device, non_blocking=True), mask.to(device, non_blocking=True)


def step(device, model, tokenizer_encoder, tokenizer_decoder,
         tokenizer_encoder_add_special_tokens: bool, tokenized_encoder_sentence_max_length: int,
         tokenizer_decoder_add_special_tokens: bool, tokenized_decoder_sentence_max_length: int,
         encoder_perturb_pct: float, decoder_perturb_pct: float, opt, lr_sched, batch,
         vocab_size_encoder: int, vocab_size_decoder: int, console=None, grad_sync=None, engine=None):
    input_ids_encoder, attention_mask_encoder = _tokenize(batch, tokenizer_encoder, tokenizer_encoder_add_special_tokens,
                                                          tokenized_encoder_sentence_max_length, device, "encoder")
    same_side = tokenizer_decoder is tokenizer_encoder and tokenizer_decoder_add_special_tokens == tokenizer_encoder_add_special_tokens \
        and tokenized_decoder_sentence_max_length == tokenized_encoder_sentence_max_length and "input_ids_decoder" not in batch
    if same_side:                                   # one tokenizer call serves both sides (bert2bert, the reference's default)
        input_ids_decoder, attention_mask_decoder = input_ids_encoder, attention_mask_encoder
    else:
        input_ids_decoder, attention_mask_decoder = _tokenize(batch, tokenizer_decoder, tokenizer_decoder_add_special_tokens,
                                                              tokenized_decoder_sentence_max_length, device, "decoder")
    input_ids_encoder = replace_pct_rand_values(input_ids_encoder, encoder_perturb_pct, 0, vocab_size_encoder)      # Trainer.py:85
    input_ids_decoder = replace_pct_rand_values(input_ids_decoder, decoder_perturb_pct, 0, vocab_size_decoder)      # Trainer.py:94
    labels = batch.get("latent_classes_labels") if isinstance(batch, dict) else None

    if engine is not None:
        # the decoder side is handed over only when it differs from the encoder's: the autoencoding step then shares one sort
        dec = {} if input_ids_decoder is input_ids_encoder else dict(dec_ids=input_ids_decoder, dec_mask=attention_mask_decoder)
        start_id = getattr(model, "decoder_next_token_start_id", None)
        if start_id is not None:
            # DECODER_NEXT_TOKEN: the decoder reads [start, ids[:-1]] and its logits at t are scored against ids[t], which it has
            # not seen (the reference scores them against the token it has just been given); nothing else in the step changes
            from kvq.functional import shift_right
            dec = dict(dec_ids=shift_right(input_ids_decoder, int(start_id)), dec_mask=shift_right(attention_mask_decoder, 1),
                       target_ids=input_ids_decoder)
        if opt is not None:
            packed = batch.get("packed") if isinstance(batch, dict) and not dec and encoder_perturb_pct == 0 else None
            out = engine.train_step(input_ids_encoder, attention_mask_encoder, prepared=packed, **dec)
        else:
            out = engine.eval_step(input_ids_encoder, attention_mask_encoder, **dec)
        loss_recon_step, acc_batch, acc_sentence, recon_ids = out["loss_recon"], out["acc"], out["acc_per_sentence"], out["recon_ids"]
    else:
        if getattr(model, "decoder_next_token_start_id", None) is not None:
            raise ValueError("DECODER_NEXT_TOKEN needs the engine step (it scores the logits against target_ids of its own)")
        pad = getattr(model, "loss_ignore_index", None)                                           # LOSS_IGNORE_PAD: the pad id
        loss_recon_step, acc_batch, recon_ids = model.forward_loss(input_ids_encoder, attention_mask_encoder,
                                                                   input_ids_decoder, attention_mask_decoder, ignore_index=pad)
        if pad is None:
            acc_sentence = torch.eq(recon_ids, input_ids_decoder).to(torch.float32).mean(dim=-1)  # common/metrics.py:32
        else:                                                                                      # over the sentence's real tokens; none: 0
            real = input_ids_decoder != pad
            acc_sentence = (torch.eq(recon_ids, input_ids_decoder) & real).sum(dim=-1) / real.sum(dim=-1).clamp(min=1)
        if opt is not None:                                                                        # Trainer.py:115-122
            grad_sync.zero_grad() if grad_sync is not None else opt.zero_grad()
            loss_recon_step.backward()
            if grad_sync is not None:
                grad_sync.finish()
            opt.step()
            if lr_sched is not None:
                lr_sched.step()
    loss_recon_step = loss_recon_step.detach()
    stats = {
        "loss_recon_step": loss_recon_step,
        "loss_full_step": loss_recon_step,                                                         # Trainer.py:111
        "metric_acc_step_per_batch": acc_batch.detach(),
        "metric_acc_step_per_sentence": acc_sentence.detach(),
        "padding_tokens_pct_step": -69,
    }
    if engine is not None and "grad_norm" in out:         # TrainEngine(max_grad_norm=...): a device scalar like the others
        stats["grad_norm_step"] = out["grad_norm"]
    if engine is not None and "optimizer_step" in out:    # grad_accum: whether this call ran the optimiser (a Python bool, no device read)
        stats["optimizer_step"] = out["optimizer_step"]
    if engine is not None and "weight_ema_decay" in out:  # weight_ema: the decay this step's update used, a device scalar like the others
        stats["weight_ema_decay_step"] = out["weight_ema_decay"]
    if engine is not None and "lr" in out:            # lr_warmup_steps / lr_decay: the rate this step was applied under, a device scalar
        stats["lr_step"] = out["lr"]
    return stats, input_ids_encoder, input_ids_decoder, recon_ids, labels


def end_of_step_stats_update(stats_stage_run: dict, stats_step: dict, n_els_batch: int):
    # LOSS_IGNORE_PAD: a step's loss and accuracy are then means over its real tokens, but the epoch means below stay weighted by
    # SENTENCES (n_els_batch), as before -- not by out["loss_tokens"]
    stats_stage_run["loss_recon_run"] += stats_step["loss_recon_step"] * n_els_batch
    stats_stage_run["loss_full_run"] += stats_step["loss_full_step"] * n_els_batch
    stats_stage_run["metric_acc_run"] += stats_step["metric_acc_step_per_batch"] * n_els_batch * 1e2
    stats_stage_run["padding_tokens_pct_run"] += stats_step["padding_tokens_pct_step"]
    grad_norm_note(stats_stage_run, stats_step)
    optimizer_step_note(stats_stage_run, stats_step)
    if "weight_ema_decay_step" in stats_step:     # the last one of the stage is what the epoch's line reports
        stats_stage_run["weight_ema_decay_last"] = stats_step["weight_ema_decay_step"]
    if "lr_step" in stats_step:                   # likewise the learning rate under a schedule: read once, at the end of the epoch
        stats_stage_run["lr_last"] = stats_step["lr_step"]
    return stats_stage_run


_LOWER_IS_BETTER = {"loss_recon": True, "loss_full": True, "metric_acc": False}


def _sum_over_ranks(stats_stage_run: dict, n_els_epoch: int):
    """Data-parallel runs: one small all-reduce per stage and epoch turns every rank's sums into sums over the whole split."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return stats_stage_run, n_els_epoch
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    keys = list(_LOWER_IS_BETTER)
    vec = torch.stack([torch.as_tensor(stats_stage_run[f"{k}_run"], dtype=torch.float64, device=dev).reshape(()) for k in keys] +
                      [torch.tensor(float(n_els_epoch), dtype=torch.float64, device=dev)])
    dist.all_reduce(vec, op=dist.ReduceOp.SUM)
    for k, v in zip(keys, vec[:-1].tolist()):
        stats_stage_run[f"{k}_run"] = v
    return stats_stage_run, int(round(vec[-1].item()))


def end_of_epoch_stats_update(stats_stage_run: dict, stats_stage_best: dict, n_els_epoch: int, n_steps: int):
    stats_stage_run, n_els_epoch = _sum_over_ranks(stats_stage_run, n_els_epoch)
    for key in _LOWER_IS_BETTER:
        stats_stage_run[f"{key}_run"] = float(stats_stage_run[f"{key}_run"]) / max(n_els_epoch, 1)      # one sync per epoch
    stats_stage_run["padding_tokens_pct_run"] /= max(n_steps, 1)
    for key, lower in _LOWER_IS_BETTER.items():
        cur, best = stats_stage_run[f"{key}_run"], stats_stage_best[f"{key}_best"]
        is_best = cur < best if lower else cur > best
        stats_stage_best[f"{key}_is_best"] = is_best
        if is_best:
            stats_stage_best[f"{key}_best"] = cur
    return stats_stage_run, stats_stage_best


def end_of_epoch_print(stats_stage_run, stats_stage_best, console, epoch, print_epoch, stat_color, stat_emojis, print_new_line):
    if console is None:
        return
    head = f"[bold {COLOR_EPOCH}]{epoch:03d}[/bold {COLOR_EPOCH}] | " if print_epoch else "    | "
    console.print(
        head +
        f"loss_recon: [bold {stat_color}] {stats_stage_run['loss_recon_run']:08.6f}[/bold {stat_color}] "
        f"{stat_emojis[1] if stats_stage_best['loss_recon_is_best'] else '  '} | "
        f"acc: [bold {stat_color}]{stats_stage_run['metric_acc_run']:08.6f}%[/bold {stat_color}] "
        f"{stat_emojis[2] if stats_stage_best['metric_acc_is_best'] else '  '} | " +
        "".join(f"{k}: [bold {stat_color}]{stats_stage_run[k]:08.6f}[/bold {stat_color}] | " for k in FR_KEYS if k in stats_stage_run) +      # FREE_RUNNING_EVAL
        ("\n" if print_new_line else ""))


def init_stats_best():
    return {"loss_recon_best": np.inf, "loss_recon_is_best": False, "loss_full_best": np.inf, "loss_full_is_best": False,
            "metric_acc_best": 0, "metric_acc_is_best": False}


def init_stats_run():
    return {"loss_recon_run": 0, "loss_full_run": 0, "metric_acc_run": 0, "padding_tokens_pct_run": 0}


def create_wandb_log_dict(epoch: int, stats_stage_run: dict, stage: str):
    rec = {"epoch": epoch, f"{stage}/loss_recon": stats_stage_run["loss_recon_run"], f"{stage}/loss_full": stats_stage_run["loss_full_run"],
           f"{stage}/acc": stats_stage_run["metric_acc_run"], f"padding_tokens_pct/{stage}": stats_stage_run["padding_tokens_pct_run"]}
    rec.update({f"{stage}/{k}": stats_stage_run[k] for k in FR_KEYS if k in stats_stage_run})      # FREE_RUNNING_EVAL: the stage's free-running numbers
    return rec


# the five generative factors the reference spells out per decoded sentence (Trainer.py:205-253): (row key, {label: name})
_EXPLICIT = [("sentence_type", {0: "declarative", 1: "interrogative"}),
             ("grammatical_number_person", {0: "1st", 1: "2nd", 2: "3rd"}),
             ("sentence_negation", {0: "affirmative", 1: "negative"}),
             ("verb_tense", {0: "past", 1: "present", 2: "future"}),
             ("sentence_style", {0: "not_progressive", 1: "progressive"})]


def explicit_latent_classes_labels(latent_classes_labels: Tensor, console=None):
    """Labels outside the reference's tables (the synthetic corpus has other factor cardinalities) are kept as their number."""
    vals = [int(v) for v in latent_classes_labels[:len(_EXPLICIT)]]
    return {key: names.get(v, str(v)) for (key, names), v in zip(_EXPLICIT, vals)}


def decode_sentences(input_ids_encoder, input_ids_decoder, recon_ids, latent_classes_labels, stats_step, tokenizer_encoder,
                     tokenizer_decoder, decoded_sentences: list, epoch: int, stage: str, console=None, free_running_rec=None):
    """free_running_rec: a TrainEngine.reconstruct(want_ids=True) result of the batch (FREE_RUNNING_EVAL) -- the rows then also carry
    free_running_sentence, free_running_edit_distance, free_running_exact."""
    def _decode(tok, ids):
        try:
            return tok.batch_decode(sequences=ids.cpu(), skip_special_tokens=True)
        except TypeError:                                           # the offline word tokenizer has no such switch
            return tok.batch_decode(ids.cpu())
    input_decoded, recon_decoded = _decode(tokenizer_encoder, input_ids_encoder), _decode(tokenizer_decoder, recon_ids)
    accs = stats_step["metric_acc_step_per_sentence"].cpu().tolist()
    labels = latent_classes_labels.cpu() if latent_classes_labels is not None else [None] * len(accs)
    extra = decoded_columns(free_running_rec, tokenizer_decoder) if free_running_rec is not None else [None] * len(accs)
    for i, r, a, l, fr in zip(input_decoded, recon_decoded, accs, labels, extra):
        row = {"epoch": epoch, "stage": stage, "input_sentence": i, "recon_sentence": r, "sentence_acc": a}
        if l is not None:
            row.update(explicit_latent_classes_labels(l, console))
        if fr is not None:
            row.update(fr)
        decoded_sentences.append(row)


def _save_ckpt(model, checkpoint_file_path: str, stage: str = ""):
    save({"model_state_dict": model.state_dict(), "encoder_state_dict": model.encoder.state_dict(),
          "decoder_state_dict": model.decoder.state_dict()}, checkpoint_file_path)


def checkpoint(stats_best: dict, model, checkpoint_dir: str, stage: str):
    if stats_best["loss_recon_is_best"]:
        _save_ckpt(model, f"{checkpoint_dir}/bagon_ckpt_loss_recon_{stage}_best.pth", stage)
    if stats_best["metric_acc_is_best"]:
        _save_ckpt(model, f"{checkpoint_dir}/bagon_ckpt_metric_acc_{stage}_best.pth", stage)


def _batch_size(batch) -> int:
    """Sentences in a batch, whichever form it takes: the DataLoader's dict of strings, the token cache's dict of ids, or
    ids tokenised per side (input_ids_encoder / input_ids_decoder, which step() accepts as well)."""
    if isinstance(batch, dict):
        if "sentence" in batch:
            return len(batch["sentence"])
        for key in ("input_ids", "input_ids_encoder", "input_ids_decoder"):
            if key in batch:
                return int(batch[key].shape[0])
        raise KeyError(f"batch without sentences or ids: keys {sorted(batch)}")
    return len(batch)


def _stage(stage, loader, n_batches, step_kw, opt, lr_sched, pcts, decode_into, epoch, grad_sync, engine, prg=None, task=None,
           free_running=None):
    """free_running: a kvq.free_running.FreeRunningEval (FREE_RUNNING_EVAL) -- the stages it runs in also generate every batch from
    its latent and compare it with the decoder's ids on the device; the stage's record gains fr_exact, fr_token_acc, fr_edit_rate."""
    run, n_els, n_steps = init_stats_run(), 0, 0
    fr_on = free_running is not None and free_running.runs(stage)
    if fr_on:
        free_running.begin()
    for batch in islice(loader, n_batches):
        n = _batch_size(batch)
        n_els += n
        n_steps += 1
        with (torch.enable_grad() if opt is not None else no_grad()):
            st, ids_enc, ids_dec, recon, labels = step(opt=opt, lr_sched=lr_sched, batch=batch, encoder_perturb_pct=pcts[0],
                                                       decoder_perturb_pct=pcts[1], grad_sync=grad_sync, engine=engine, **step_kw)
        fr_rec = None
        if fr_on:       # the ids are the step's (perturbed as scored); the masks are the batch's
            dev = step_kw["device"]
            m_enc = _tokenize(batch, step_kw["tokenizer_encoder"], step_kw["tokenizer_encoder_add_special_tokens"],
                              step_kw["tokenized_encoder_sentence_max_length"], dev, "encoder")[1]
            m_dec = m_enc if ids_dec is ids_enc else _tokenize(batch, step_kw["tokenizer_decoder"], step_kw["tokenizer_decoder_add_special_tokens"],
                                                               step_kw["tokenized_decoder_sentence_max_length"], dev, "decoder")[1]
            with no_grad():
                fr_rec = free_running.batch(ids_enc, m_enc, None if ids_dec is ids_enc else ids_dec, None if ids_dec is ids_enc else m_dec,
                                            labels=labels, want_ids=decode_into is not None)
        if decode_into is not None:
            decode_sentences(ids_enc, ids_dec, recon, labels, st, step_kw["tokenizer_encoder"], step_kw["tokenizer_decoder"],
                             decode_into, epoch, stage, step_kw.get("console"), free_running_rec=fr_rec)
        run = end_of_step_stats_update(run, st, n)
        if prg is not None and task is not None:
            prg.advance(task, 1)
    if fr_on:
        run.update(free_running.finish())          # one read of the census, at the end of the stage
    return run, n_els, n_steps


def train(prg, console, device, dl_train, dl_val, n_batches_train, n_batches_val, model, tokenizer_encoder, tokenizer_decoder,
          tokenizer_encoder_add_special_tokens, tokenized_encoder_sentence_max_length,
          tokenizer_decoder_add_special_tokens, tokenized_decoder_sentence_max_length,
          encoder_perturb_train_pct, encoder_perturb_val_pct, decoder_perturb_train_pct, decoder_perturb_val_pct,
          n_epochs_to_decode_after, decoded_sentences, opt, lr_sched, n_epochs, vocab_size_encoder, vocab_size_decoder,
          wandb_run, run_path, export_checkpoint=True, grad_sync=None, engine=None, is_main=True,
          train_state_path=None, train_state_every: int = 1, resume=None, train_state_config=None, weight_ema_eval: bool = True,
          free_running=None):
    """free_running: a kvq.free_running.FreeRunningEval whose validation switch is on makes every validation stage report the
    free-running numbers too (the best-checkpoint decision does not read them).
    weight_ema_eval: with an engine that keeps an average of the weights (TrainEngine(weight_ema=...)), run every validation
    stage under it and write the best-val checkpoints while it is applied: they hold the weights that were scored.
    train_state_path: the run's training-state file (kvq.train_state; None: none is written), rewritten at the end of every
    train_state_every-th epoch and of the last one, behind validation and the best checkpoints.  resume: such a file's dict
    (load_train_state) -- the loop starts behind its last finished epoch; model and engine / optimiser were loaded by the caller.
    train_state_config: the run's configuration, stored in the file."""
    check_every(train_state_every, "train_state_every")
    stats_train_best, stats_val_best = init_stats_best(), init_stats_best()
    step_kw = dict(device=device, model=model, tokenizer_encoder=tokenizer_encoder, tokenizer_decoder=tokenizer_decoder,
                   tokenizer_encoder_add_special_tokens=tokenizer_encoder_add_special_tokens,
                   tokenized_encoder_sentence_max_length=tokenized_encoder_sentence_max_length,
                   tokenizer_decoder_add_special_tokens=tokenizer_decoder_add_special_tokens,
                   tokenized_decoder_sentence_max_length=tokenized_decoder_sentence_max_length,
                   vocab_size_encoder=vocab_size_encoder, vocab_size_decoder=vocab_size_decoder, console=console)
    tasks = None
    if prg is not None:
        prg.start()
        tasks = (prg.add_task(f"[bold {COLOR_TRAIN}] Train batches", total=n_batches_train),
                 prg.add_task(f"[bold {COLOR_VAL}] Val   batches", total=n_batches_val))
    hist = []
    skipped = 0
    first_epoch = 1
    if resume is not None:
        first_epoch, stats_train_best, stats_val_best, hist, skipped = restore_trainer(resume, decoded_sentences, dl_train)
    if console is not None and param_groups_line(engine) is not None:      # param_groups: the resolved table, once per run
        console.print("    | " + param_groups_line(engine))
    for epoch in range(first_epoch, n_epochs + 1):
        if prg is not None:
            prg.reset(tasks[0]); prg.reset(tasks[1])
        dec = decoded_sentences if epoch % n_epochs_to_decode_after == 0 else None
        model.train()
        t_stage = _time.perf_counter()
        run, n, s = _stage("train", dl_train, n_batches_train, step_kw, opt, lr_sched,
                           (encoder_perturb_train_pct, decoder_perturb_train_pct), dec, epoch, grad_sync, engine, prg, tasks and tasks[0])
        stats_train_run, stats_train_best = end_of_epoch_stats_update(run, stats_train_best, n, s)
        guard_rec, skipped = grad_guard_epoch_record(engine, run, s, skipped)             # max_grad_norm: mean norm, skipped steps
        if guard_rec is not None:
            wandb_run.log({"epoch": epoch, **guard_rec})
            if console is not None:
                console.print(f"    | grad_norm: {guard_rec['train/grad_norm']:.6f} | skipped steps: {guard_rec['train/skipped_steps']}")
        n_opt = optimizer_steps_epoch(run, s)                                             # grad_accum: a cycle left open carries into the next epoch
        wema_rec = weight_ema_epoch_record(engine, run.pop("weight_ema_decay_last", None))      # weight_ema: decay in force, updates so far
        if wema_rec is not None:
            wandb_run.log({"epoch": epoch, **wema_rec})
            if console is not None:
                console.print(f"    | weight EMA decay: {wema_rec['train/weight_ema_decay']} | updates: {wema_rec['train/weight_ema_updates']}"
                              f"{'' if weight_ema_eval else ' | evaluation on the live weights'}")
        lr_rec = lr_epoch_record(engine, run.pop("lr_last", None))                        # lr schedule: the epoch's last rate
        if lr_rec is not None:
            wandb_run.log({"epoch": epoch, **lr_rec})
            if console is not None:
                console.print(f"    | lr: {lr_rec['train/lr']:.6e}")
        # sentences/s of THIS rank's train stage, loop and all (end_of_epoch_stats_update has just turned the device sums into
        # floats: the stage's kernels have finished).  An extra log entry, not one of the reference's keys.
        wandb_run.log({"epoch": epoch, "perf/train_s": _time.perf_counter() - t_stage, "perf/train_steps": s, "perf/optimizer_steps": n_opt,
                       "perf/train_sentences_per_s": n / max(_time.perf_counter() - t_stage, 1e-9)})
        end_of_epoch_print(stats_train_run, stats_train_best, console, epoch, True, COLOR_TRAIN, STATS_EMOJI_TRAIN, False)
        wandb_run.log(create_wandb_log_dict(epoch, stats_train_run, "train"))
        if export_checkpoint and is_main:
            checkpoint(stats_train_best, model, run_path, "train")
        model.eval()
        with weight_ema_scope(engine, weight_ema_eval):       # weight_ema: validation and the best-val checkpoints under the average
            run, n, s = _stage("val", dl_val, n_batches_val, step_kw, None, None, (encoder_perturb_val_pct, decoder_perturb_val_pct),
                               dec, epoch, None, engine, prg, tasks and tasks[1], free_running=free_running)
            stats_val_run, stats_val_best = end_of_epoch_stats_update(run, stats_val_best, n, s)
            end_of_epoch_print(stats_val_run, stats_val_best, console, epoch, False, COLOR_VAL, STATS_EMOJI_VAL, epoch != n_epochs)
            wandb_run.log(create_wandb_log_dict(epoch, stats_val_run, "val"))
            if export_checkpoint and is_main:
                checkpoint(stats_val_best, model, run_path, "val")
        hist.append((stats_train_run, stats_val_run))
        if train_state_path is not None and (epoch % train_state_every == 0 or epoch == n_epochs):
            # (before drop_open_accumulation: a cycle the last epoch left open travels in the file and continues in a resumed run)
            save_train_state(train_state_path, model, trainer_state(epoch, stats_train_best, stats_val_best, hist, skipped,
                                                                    decoded_sentences, dl_train),
                             train_state_config or {}, engine=engine, opt=opt, lr_sched=lr_sched, is_main=is_main)
    drop_open_accumulation(engine, console)
    if prg is not None:
        prg.stop()
    return hist


def test(prg, console, device, dl_test, n_batches_test, model, tokenizer_encoder, tokenizer_decoder,
         tokenizer_encoder_add_special_tokens, tokenized_encoder_sentence_max_length,
         tokenizer_decoder_add_special_tokens, tokenized_decoder_sentence_max_length,
         encoder_perturb_test_pct, decoder_perturb_test_pct, decoded_sentences, vocab_size_encoder, vocab_size_decoder, epoch,
         wandb_run, engine=None, weight_ema_eval: bool = True, free_running=None):
    """free_running: a kvq.free_running.FreeRunningEval -- the stage also measures free-running reconstruction (FREE_RUNNING_EVAL).
    weight_ema_eval: with an engine that keeps an average of the weights, score the test split under it (False: under the
    weights the model holds -- what a caller passes who has just loaded a checkpoint that already holds the average)."""
    step_kw = dict(device=device, model=model, tokenizer_encoder=tokenizer_encoder, tokenizer_decoder=tokenizer_decoder,
                   tokenizer_encoder_add_special_tokens=tokenizer_encoder_add_special_tokens,
                   tokenized_encoder_sentence_max_length=tokenized_encoder_sentence_max_length,
                   tokenizer_decoder_add_special_tokens=tokenizer_decoder_add_special_tokens,
                   tokenized_decoder_sentence_max_length=tokenized_decoder_sentence_max_length,
                   vocab_size_encoder=vocab_size_encoder, vocab_size_decoder=vocab_size_decoder, console=console)
    model.eval()
    with weight_ema_scope(engine, weight_ema_eval):
        run, n, s = _stage("test", dl_test, n_batches_test, step_kw, None, None, (encoder_perturb_test_pct, decoder_perturb_test_pct),
                           decoded_sentences, epoch, None, engine, free_running=free_running)
    stats_test_run, stats_test_best = end_of_epoch_stats_update(run, init_stats_best(), n, s)
    end_of_epoch_print(stats_test_run, stats_test_best, console, epoch, False, COLOR_TEST, STATS_EMOJI_TEST, True)
    wandb_run.log(create_wandb_log_dict(epoch, stats_test_run, "test"))
    return stats_test_run
