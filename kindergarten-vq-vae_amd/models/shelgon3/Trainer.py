"""step / train / test of the Shelgon (VQ) run -- counterpart of models/shelgon3/Trainer.py:65-462.

Kept: the function names and argument lists, the per-step stats dict and its keys, running / best bookkeeping,
checkpoint file names and dict keys (`model_state_dict`, `encoder_state_dict`, `decoder_state_dict`), the per-STEP
scheduler tick, validation under no_grad with opt=None.

Changed on purpose (hot path):
  * the loss block `kl_div(log_softmax(logits), one_hot(ids))` + `argmax(softmax(logits))` + `seq_acc`
    (Trainer.py:94-101) is one fused kernel pass over the logits (Shelgon.forward_loss -> kvq_ce_forward);
  * stats stay on the device (no .item() per step), batches are consumed lazily instead of `list(dl_train)`;
  * optional `grad_sync` (kvq.ddp.GradSync) overlaps the RCCL gradient all-reduce with backward.
Deviations from reference quirks, documented: running means are weighted by the true batch size (the reference
weights by len(batch-dict) == 2, which cancels out), `metric_acc_step` is the per-batch accuracy (the reference
stores the (batch, per-sentence) tuple by mistake), the "val" checkpoint is decided by the VAL best flags.
"""
from __future__ import annotations

import time as _time
from itertools import islice
from math import isclose

import numpy as np
import torch
from torch import Tensor, no_grad, save

from common.consts import *  # noqa: F401,F403  (colours / emoji)
from kvq.runlog import (codes_revived_note, drop_open_accumulation, grad_guard_epoch_record, grad_norm_note, optimizer_step_note,
                        optimizer_steps_epoch, revive_epoch_record, weight_ema_epoch_record, weight_ema_scope, lr_epoch_record, param_groups_line)
from kvq.free_running import FR_KEYS, decoded_columns
from kvq.train_state import check_every, restore_trainer, save_train_state, trainer_state


def tokenize_batch(batch, tokenizer, tokenizer_add_special_tokens: bool, max_length: int, device):
    """Trainer.py:78-84.  Batches that already carry `input_ids` (pre-tokenised cache) skip the tokenizer."""
    if "input_ids" in batch:
        ids, mask = batch["input_ids"], batch["attention_mask"]
    else:
        tok = tokenizer(batch["sentence"], return_tensors="pt", padding="max_length", max_length=max_length,
                        add_special_tokens=tokenizer_add_special_tokens)
        ids, mask = tok.input_ids, tok.attention_mask
    return ids.to(device, non_blocking=True), mask.to(device, non_blocking=True)


def step(device, model, tokenizer, tokenizer_add_special_tokens: bool, opt,
         loss_recon_rescale_factor: float, loss_recon_weight: float,
         loss_vq_rescale_factor: float, loss_vq_weight: float,
         loss_perp_rescale_factor: float, loss_perp_weight: float,
         lr_sched, batch, vocab_size: int, stage: str, console=None, max_length: int = 12, grad_sync=None, engine=None):
    input_ids, attention_mask = tokenize_batch(batch, tokenizer, tokenizer_add_special_tokens, max_length, device)

    if engine is not None:
        # fast path: kvq.engine.TrainEngine runs forward, backward, gradient exchange and Adam (+ the per-step scheduler
        # tick) itself; the loss weights were given to its constructor
        start_id = getattr(model, "decoder_next_token_start_id", None)
        if start_id is not None:
            # DECODER_NEXT_TOKEN: the decoder reads [start, ids[:-1]] and its logits at t are scored against ids[t], which it has
            # not seen (the reference scores them against the token it has just been given); nothing else in the step changes
            from kvq.functional import shift_right
            dec = dict(dec_ids=shift_right(input_ids, int(start_id)), dec_mask=shift_right(attention_mask, 1), target_ids=input_ids)
            out = engine.train_step(input_ids, attention_mask, **dec) if opt is not None else engine.eval_step(input_ids, attention_mask, **dec)
        else:
            out = engine.train_step(input_ids, attention_mask, prepared=batch.get("packed") if isinstance(batch, dict) else None) \
                if opt is not None else engine.eval_step(input_ids, attention_mask)
        stats = {
            "loss_recon_step": out["loss_recon"].detach(), "loss_vq_step": out["loss_vq"].detach(),
            "metric_perp_step": out["perplexity"].detach(), "loss_full_step": (out["loss_recon"] + out["loss_vq"]).detach(),
            "metric_acc_step": out["acc"].detach(), "padding_tokens_pct_step": -69,
        }
        if "grad_norm" in out:                    # TrainEngine(max_grad_norm=...): a device scalar like the others
            stats["grad_norm_step"] = out["grad_norm"]
        if "codes_revived" in out:                # revive_after: codes restarted by this step, a device scalar like the others
            stats["codes_revived_step"] = out["codes_revived"]
        if "optimizer_step" in out:               # grad_accum: whether this call ran the optimiser (a Python bool, no device read)
            stats["optimizer_step"] = out["optimizer_step"]
        if "weight_ema_decay" in out:             # weight_ema: the decay this step's update used, a device scalar like the others
            stats["weight_ema_decay_step"] = out["weight_ema_decay"]
        if "lr" in out:                           # lr_warmup_steps / lr_decay: the rate this step was applied under, a device scalar
            stats["lr_step"] = out["lr"]
        return stats, input_ids, out["recon_ids"]

    if getattr(model, "decoder_next_token_start_id", None) is not None:
        raise ValueError("DECODER_NEXT_TOKEN needs the engine step (it scores the logits against target_ids of its own)")
    loss_vq_step, metric_perp_step, _indices, loss_recon_step, acc_step, recon_ids = \
        model.forward_loss(input_ids, attention_mask, ignore_index=getattr(model, "loss_ignore_index", None))      # LOSS_IGNORE_PAD: the pad id

    loss_recon_step = loss_recon_step * (loss_recon_rescale_factor * loss_recon_weight)      # Trainer.py:103
    loss_vq_step = loss_vq_step * (loss_vq_rescale_factor * loss_vq_weight)                  # Trainer.py:104
    loss_full_step: Tensor = loss_recon_step + loss_vq_step                                  # Trainer.py:105

    if opt is not None:                                                                       # Trainer.py:109-115
        if grad_sync is not None:
            grad_sync.zero_grad()
        else:
            opt.zero_grad()
        loss_full_step.backward()
        if grad_sync is not None:
            grad_sync.finish()
        opt.step()
        if lr_sched is not None:
            lr_sched.step()

    return {
        "loss_recon_step": loss_recon_step.detach(),
        "loss_vq_step": loss_vq_step.detach(),
        "metric_perp_step": metric_perp_step.detach(),
        "loss_full_step": loss_full_step.detach(),
        "metric_acc_step": acc_step.detach(),
        "padding_tokens_pct_step": -69,
    }, input_ids, recon_ids


def end_of_step_stats_update(stats_stage_run: dict, stats_step: dict, n_els_batch: int):
    # LOSS_IGNORE_PAD: a step's loss and accuracy are then means over its real tokens, but the epoch means below stay weighted by
    # SENTENCES (n_els_batch), as before -- not by out["loss_tokens"]
    stats_stage_run["loss_recon_run"] += stats_step["loss_recon_step"] * n_els_batch
    stats_stage_run["loss_vq_run"] += stats_step["loss_vq_step"] * n_els_batch
    stats_stage_run["metric_perp_run"] += stats_step["metric_perp_step"] * n_els_batch
    stats_stage_run["loss_full_run"] += stats_step["loss_full_step"] * n_els_batch
    stats_stage_run["metric_acc_run"] += stats_step["metric_acc_step"] * n_els_batch * 1e2
    stats_stage_run["padding_tokens_pct_run"] += stats_step["padding_tokens_pct_step"]
    grad_norm_note(stats_stage_run, stats_step)
    codes_revived_note(stats_stage_run, stats_step)
    optimizer_step_note(stats_stage_run, stats_step)
    if "weight_ema_decay_step" in stats_step:     # the last one of the stage is what the epoch's line reports
        stats_stage_run["weight_ema_decay_last"] = stats_step["weight_ema_decay_step"]
    if "lr_step" in stats_step:                   # likewise the learning rate under a schedule: read once, at the end of the epoch
        stats_stage_run["lr_last"] = stats_step["lr_step"]
    return stats_stage_run


_LOWER_IS_BETTER = {"loss_recon": True, "loss_vq": True, "metric_perp": False, "loss_full": True, "metric_acc": False}


def _sum_over_ranks(stats_stage_run: dict, n_els_epoch: int):
    """Data-parallel runs: every rank has accumulated the sums of ITS shard; one small all-reduce per stage and epoch turns
    them into sums over the whole split, so the printed / logged means and the best-checkpoint decision are the ones a single
    process on the global batch would make (the reference is single-process, Trainer.py:127-143)."""
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
        stats_stage_run[f"{key}_run"] = float(stats_stage_run[f"{key}_run"]) / max(n_els_epoch, 1)   # one sync per epoch
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

    def cell(label, key, emoji, pct=""):
        mark = emoji if stats_stage_best[f"{key}_is_best"] else "  "
        return f"{label}: [bold {stat_color}] {stats_stage_run[key + '_run']:08.6f}{pct}[/bold {stat_color}] {mark} | "

    line = head + cell("loss_recon", "loss_recon", stat_emojis[1]) + cell("loss_vq", "loss_vq", stat_emojis[0])
    if not isclose(stats_stage_run["metric_perp_run"], -69):
        line += cell("perp", "metric_perp", stat_emojis[3])
    line += cell("acc", "metric_acc", stat_emojis[2], "%")
    line += "".join(f"{k}: [bold {stat_color}] {stats_stage_run[k]:08.6f}[/bold {stat_color}] | " for k in FR_KEYS if k in stats_stage_run)      # FREE_RUNNING_EVAL
    console.print(line + ("\n" if print_new_line else ""))


def init_stats_best():
    return {"loss_recon_best": np.inf, "loss_recon_is_best": False, "loss_vq_best": np.inf, "loss_vq_is_best": False,
            "metric_perp_best": 0, "metric_perp_is_best": False, "loss_full_best": np.inf, "loss_full_is_best": False,
            "metric_acc_best": 0, "metric_acc_is_best": False}


def init_stats_run():
    return {"loss_recon_run": 0, "loss_vq_run": 0, "metric_perp_run": 0, "loss_full_run": 0, "metric_acc_run": 0,
            "padding_tokens_pct_run": 0}


def create_wandb_log_dict(epoch: int, stats_stage_run: dict, stage: str):
    rec = {"epoch": epoch,
           f"{stage}/loss_recon": stats_stage_run["loss_recon_run"], f"{stage}/loss_vq": stats_stage_run["loss_vq_run"],
           f"{stage}/metric_perp": stats_stage_run["metric_perp_run"], f"{stage}/loss_full": stats_stage_run["loss_full_run"],
           f"{stage}/acc": stats_stage_run["metric_acc_run"],
           f"padding_tokens_pct/{stage}": stats_stage_run["padding_tokens_pct_run"]}
    rec.update({f"{stage}/{k}": stats_stage_run[k] for k in FR_KEYS if k in stats_stage_run})      # FREE_RUNNING_EVAL: the stage's free-running numbers
    return rec


def decode_sentences(input_ids, recon_ids, tokenizer, decoded_sentences: list, epoch: int, stage: str, console=None, free_running_rec=None):
    """free_running_rec: a TrainEngine.reconstruct(want_ids=True) result of the batch (FREE_RUNNING_EVAL) -- the rows then also carry
    free_running_sentence, free_running_edit_distance, free_running_exact."""
    extra = decoded_columns(free_running_rec, tokenizer) if free_running_rec is not None else [None] * int(input_ids.shape[0])
    for i, r, fr in zip(tokenizer.batch_decode(sequences=input_ids.cpu()), tokenizer.batch_decode(sequences=recon_ids.cpu()), extra):
        row = {"epoch": epoch, "stage": stage, "input_sentence": i, "recon_sentence": r}
        if fr is not None:
            row.update(fr)
        decoded_sentences.append(row)


def _save_ckpt(model, checkpoint_file_path: str, stage: str):
    save({"model_state_dict": model.state_dict(), "encoder_state_dict": model.encoder.state_dict(),
          "decoder_state_dict": model.decoder.state_dict()}, checkpoint_file_path)        # Trainer.py:240-249


def checkpoint(stats_best: dict, model, checkpoint_dir: str, stage: str):
    if stats_best["loss_recon_is_best"]:
        _save_ckpt(model, f"{checkpoint_dir}/shelgon_ckpt_loss_recon_{stage}_best.pth", stage)
    if stats_best["loss_vq_is_best"]:
        _save_ckpt(model, f"{checkpoint_dir}/shelgon_ckpt_loss_vq_{stage}_best.pth", stage)


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


def _run_stage(stage, device, loader, n_batches, model, tokenizer, tokenizer_add_special_tokens, opt, lr_sched, weights,
               vocab_size, decode_into, epoch, console, max_length, grad_sync, on_batch=None, engine=None, free_running=None):
    """free_running: a kvq.free_running.FreeRunningEval (FREE_RUNNING_EVAL) -- the stages it runs in also generate every batch from
    its latent and compare it with the input on the device; the stage's record gains fr_exact, fr_token_acc, fr_edit_rate."""
    stats_run = init_stats_run()
    n_els_epoch = n_steps = 0
    fr_on = free_running is not None and free_running.runs(stage)
    if fr_on:
        free_running.begin()
    for batch in islice(loader, n_batches):
        n_els_batch = _batch_size(batch)
        n_els_epoch += n_els_batch
        n_steps += 1
        ctx = torch.enable_grad() if opt is not None else no_grad()
        with ctx:
            stats_step, input_ids, recon_ids = step(
                device=device, model=model, tokenizer=tokenizer, tokenizer_add_special_tokens=tokenizer_add_special_tokens,
                opt=opt, lr_sched=lr_sched, batch=batch, vocab_size=vocab_size, stage=stage, console=console,
                max_length=max_length, grad_sync=grad_sync, engine=engine, **weights)
        fr_rec = None
        if fr_on:
            mask = tokenize_batch(batch, tokenizer, tokenizer_add_special_tokens, max_length, device)[1]
            with no_grad():
                fr_rec = free_running.batch(input_ids, mask, labels=batch.get("latent_classes_labels") if isinstance(batch, dict) else None,
                                            want_ids=decode_into is not None)
        if decode_into is not None:
            decode_sentences(input_ids, recon_ids, tokenizer, decode_into, epoch, stage, console, free_running_rec=fr_rec)
        stats_run = end_of_step_stats_update(stats_run, stats_step, n_els_batch)
        if on_batch:
            on_batch()
    if fr_on:
        stats_run.update(free_running.finish())          # one read of the census, at the end of the stage
    return stats_run, n_els_epoch, n_steps


def train(prg, console, device, dl_train, dl_val, n_batches_train: int, n_batches_val: int, model, tokenizer,
          tokenizer_add_special_tokens: bool, n_epochs_to_decode_after: int, decoded_sentences: list, opt,
          loss_recon_rescale_factor: float, loss_recon_weight: float, loss_vq_rescale_factor: float, loss_vq_weight: float,
          loss_perp_rescale_factor: float, loss_perp_weight: float, lr_sched, n_epochs: int, vocab_size: int,
          wandb_run, run_path: str, export_checkpoint: bool, max_length: int = 12, grad_sync=None, is_main: bool = True,
          engine=None, train_state_path=None, train_state_every: int = 1, resume=None, train_state_config=None,
          weight_ema_eval: bool = True, free_running=None):
    """free_running: a kvq.free_running.FreeRunningEval whose validation switch is on makes every validation stage report the
    free-running numbers too (the best-checkpoint decision does not read them).
    weight_ema_eval: with an engine that keeps an average of the weights (TrainEngine(weight_ema=...)), run every validation
    stage under it and write the best-val checkpoints while it is applied: they hold the weights that were scored.
    train_state_path: the run's training-state file (kvq.train_state; None: none is written), rewritten at the end of every
    train_state_every-th epoch and of the last one, behind validation and the best checkpoints.  resume: such a file's dict
    (load_train_state) -- the loop starts behind its last finished epoch; model and engine / optimiser were loaded by the caller.
    train_state_config: the run's configuration, stored in the file."""
    check_every(train_state_every, "train_state_every")
    if not export_checkpoint and console is not None:
        console.print(f"[bold {COLOR_WARNING}]Warning[/bold {COLOR_WARNING}] checkpoint exporting is [bold {COLOR_OFF}]OFF[/bold {COLOR_OFF}]!\n")
    weights = dict(loss_recon_rescale_factor=loss_recon_rescale_factor, loss_recon_weight=loss_recon_weight,
                   loss_vq_rescale_factor=loss_vq_rescale_factor, loss_vq_weight=loss_vq_weight,
                   loss_perp_rescale_factor=loss_perp_rescale_factor, loss_perp_weight=loss_perp_weight)
    tasks = None
    if prg is not None:
        prg.start()
        tasks = (prg.add_task(f"[bold {COLOR_EPOCH}] Epochs", total=n_epochs),
                 prg.add_task(f"[bold {COLOR_TRAIN}] Train batches", total=n_batches_train),
                 prg.add_task(f"[bold {COLOR_VAL}] Val   batches", total=n_batches_val))
    stats_train_best, stats_val_best = init_stats_best(), init_stats_best()
    history = []
    skipped = 0
    first_epoch = 1
    if resume is not None:
        first_epoch, stats_train_best, stats_val_best, history, skipped = restore_trainer(resume, decoded_sentences, dl_train)
    if console is not None and param_groups_line(engine) is not None:      # param_groups: the resolved table, once per run
        console.print("    | " + param_groups_line(engine))
    for epoch in range(first_epoch, n_epochs + 1):
        if tasks:
            prg.reset(tasks[1]); prg.reset(tasks[2])
        decode_now = decoded_sentences if epoch % n_epochs_to_decode_after == 0 else None

        model.train()
        tick = (lambda: (prg.advance(tasks[1], 1), prg.advance(tasks[0], 1 / (n_batches_train + n_batches_val)))) if tasks else None
        t_stage = _time.perf_counter()
        run, n_els, n_steps = _run_stage("train", device, dl_train, n_batches_train, model, tokenizer, tokenizer_add_special_tokens,
                                         opt, lr_sched, weights, vocab_size, decode_now, epoch, console, max_length, grad_sync, tick,
                                         engine=engine)
        stats_train_run, stats_train_best = end_of_epoch_stats_update(run, stats_train_best, n_els, n_steps)
        guard_rec, skipped = grad_guard_epoch_record(engine, run, n_steps, skipped)       # max_grad_norm: mean norm, skipped steps
        if guard_rec is not None:
            wandb_run.log({"epoch": epoch, **guard_rec})
            if console is not None:
                console.print(f"    | grad_norm: {guard_rec['train/grad_norm']:.6f} | skipped steps: {guard_rec['train/skipped_steps']}")
        n_opt = optimizer_steps_epoch(run, n_steps)                                       # grad_accum: a cycle left open carries into the next epoch
        revive_rec = revive_epoch_record(engine, run)                                     # revive_after: codes restarted this epoch / so far
        if revive_rec is not None:
            wandb_run.log({"epoch": epoch, **revive_rec})
            if console is not None:
                console.print(f"    | codes revived: {revive_rec['train/codes_revived']} | so far: {revive_rec['train/codes_revived_total']}")
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
        wandb_run.log({"epoch": epoch, "perf/train_s": _time.perf_counter() - t_stage, "perf/train_steps": n_steps, "perf/optimizer_steps": n_opt,
                       "perf/train_sentences_per_s": n_els / max(_time.perf_counter() - t_stage, 1e-9)})
        end_of_epoch_print(stats_train_run, stats_train_best, console, epoch, True, COLOR_TRAIN, STATS_EMOJI_TRAIN, False)
        wandb_run.log(create_wandb_log_dict(epoch, stats_train_run, "train"))

        model.eval()
        tick = (lambda: (prg.advance(tasks[2], 1), prg.advance(tasks[0], 1 / (n_batches_train + n_batches_val)))) if tasks else None
        with weight_ema_scope(engine, weight_ema_eval):       # weight_ema: validation and the best-val checkpoints under the average
            run, n_els, n_steps = _run_stage("val", device, dl_val, n_batches_val, model, tokenizer, tokenizer_add_special_tokens,
                                             None, None, weights, vocab_size, decode_now, epoch, console, max_length, None, tick,
                                             engine=engine, free_running=free_running)
            stats_val_run, stats_val_best = end_of_epoch_stats_update(run, stats_val_best, n_els, n_steps)
            end_of_epoch_print(stats_val_run, stats_val_best, console, epoch, False, COLOR_VAL, STATS_EMOJI_VAL, epoch != n_epochs)
            wandb_run.log(create_wandb_log_dict(epoch, stats_val_run, "val"))
            if export_checkpoint and is_main:
                checkpoint(stats_val_best, model, run_path, "val")
        history.append((dict(stats_train_run), dict(stats_val_run)))
        if train_state_path is not None and (epoch % train_state_every == 0 or epoch == n_epochs):
            # (before drop_open_accumulation: a cycle the last epoch left open travels in the file and continues in a resumed run)
            save_train_state(train_state_path, model, trainer_state(epoch, stats_train_best, stats_val_best, history, skipped,
                                                                    decoded_sentences, dl_train),
                             train_state_config or {}, engine=engine, opt=opt, lr_sched=lr_sched, is_main=is_main)
    drop_open_accumulation(engine, console)
    return history


def test(prg, console, device, dl_test, n_batches_test, model, tokenizer, tokenizer_add_special_tokens: bool,
         loss_recon_rescale_factor: float, loss_recon_weight: float, loss_vq_rescale_factor: float, loss_vq_weight: float,
         loss_perp_rescale_factor: float, loss_perp_weight: float, decoded_sentences: list, vocab_size: int, epoch: int,
         wandb_run, max_length: int = 12, engine=None, weight_ema_eval: bool = True, free_running=None):
    """free_running: a kvq.free_running.FreeRunningEval -- the stage also measures free-running reconstruction (FREE_RUNNING_EVAL).
    weight_ema_eval: with an engine that keeps an average of the weights, score the test split under it (False: under the
    weights the model holds -- what a caller passes who has just loaded a checkpoint that already holds the average)."""
    weights = dict(loss_recon_rescale_factor=loss_recon_rescale_factor, loss_recon_weight=loss_recon_weight,
                   loss_vq_rescale_factor=loss_vq_rescale_factor, loss_vq_weight=loss_vq_weight,
                   loss_perp_rescale_factor=loss_perp_rescale_factor, loss_perp_weight=loss_perp_weight)
    task = prg.add_task(f"[bold {COLOR_TEST}] Test  batches", total=n_batches_test) if prg is not None else None
    model.eval()
    with weight_ema_scope(engine, weight_ema_eval):
        run, n_els, n_steps = _run_stage("test", device, dl_test, n_batches_test, model, tokenizer, tokenizer_add_special_tokens,
                                         None, None, weights, vocab_size, decoded_sentences, epoch, console, max_length, None,
                                         (lambda: prg.advance(task, 1)) if task is not None else None, engine=engine,
                                         free_running=free_running)
    stats_test_run, stats_test_best = end_of_epoch_stats_update(run, init_stats_best(), n_els, n_steps)
    end_of_epoch_print(stats_test_run, stats_test_best, console, epoch, False, COLOR_TEST, STATS_EMOJI_TEST, True)
    wandb_run.log(create_wandb_log_dict(epoch, stats_test_run, "test"))
    return stats_test_run
