"""Run logging: the `wandb_run.log(dict)` / `.watch` surface the trainers call (models/shelgon3/Trainer.py:345),
backed by wandb when it is installed and WANDB_MODE is not "disabled", by a JSONL file otherwise."""
from __future__ import annotations

import json
import os
import time


class JsonlRun:
    def __init__(self, run_path: str, config: dict | None = None):
        self.path = os.path.join(run_path, "metrics.jsonl") if run_path else None
        self.config = config or {}
        self.history = []

    def log(self, record: dict):
        rec = {k: (float(v) if hasattr(v, "__float__") else v) for k, v in record.items()}
        rec["_time"] = time.time()
        self.history.append(rec)
        if self.path:
            with open(self.path, "a") as fp:
                fp.write(json.dumps(rec) + "\n")

    def watch(self, *_a, **_k):
        pass

    def log_code(self, *_a, **_k):
        pass

    def finish(self):
        pass


def init_run(project, group, job_type, config, mode, run_path):
    if mode != "disabled":
        try:
            import wandb
            return wandb.init(project=project, group=group, job_type=job_type, config=config, mode=mode)
        except ImportError:
            pass
    return JsonlRun(run_path, config)


# ---- TrainEngine(max_grad_norm=...): the step's gradient norm and the skipped steps in the trainers' logs -------------------------
def grad_norm_note(stats_stage_run: dict, stats_step: dict):
    """Add the step's global gradient norm ("grad_norm_step": a device scalar of train_step's result, present only with the option
    on) to the stage's running sum.  A skipped step's inf / NaN counts as 0.  Device arithmetic only: no synchronisation."""
    gn = stats_step.get("grad_norm_step")
    if gn is not None:
        import torch
        stats_stage_run["grad_norm_run"] = stats_stage_run.get("grad_norm_run", 0) + torch.nan_to_num(gn.float(), nan=0.0, posinf=0.0,
                                                                                                      neginf=0.0)


def grad_guard_epoch_record(engine, stats_stage_run: dict, n_steps: int, skipped_before: int, stage: str = "train"):
    """End of a training stage, after its statistics were read (the one synchronisation of the epoch): ({"<stage>/grad_norm": mean
    norm over the applied steps, "<stage>/skipped_steps": steps skipped so far} | None with the option off, steps skipped so far)."""
    total = stats_stage_run.pop("grad_norm_run", None)
    n_steps = stats_stage_run.get("optimizer_steps_run", n_steps)      # grad_accum > 1: a norm exists per OPTIMISER step, not per call
    if engine is None or getattr(engine, "max_grad_norm", None) is None or total is None:
        return None, skipped_before
    skipped = int(engine.skipped_steps)
    applied = max(n_steps - (skipped - skipped_before), 1)
    return {f"{stage}/grad_norm": float(total) / applied, f"{stage}/skipped_steps": skipped}, skipped


# ---- TrainEngine(grad_accum=...): calls of train_step against optimiser steps ------------------------------------------------------
def optimizer_step_note(stats_stage_run: dict, stats_step: dict):
    """Count the step if it ran the optimiser ("optimizer_step": the Python bool of train_step's result; a step without the key --
    evaluation, the autograd path -- is not counted).  Host arithmetic only."""
    ran = stats_step.get("optimizer_step")
    if ran is not None:
        stats_stage_run["optimizer_steps_run"] = stats_stage_run.get("optimizer_steps_run", 0) + int(bool(ran))


def optimizer_steps_epoch(stats_stage_run: dict, n_steps: int) -> int:
    """End of a training stage, behind grad_guard_epoch_record: the optimiser steps of the stage (n_steps, the number of calls,
    where no step carried the key)."""
    return int(stats_stage_run.pop("optimizer_steps_run", n_steps))


def drop_open_accumulation(engine, console=None) -> int:
    """End of train(): a cycle of micro-batches that the last epoch left open is dropped (its gradients never reach the weights);
    one console line says so.  Returns the micro-batches dropped."""
    n = int(getattr(engine, "accum_pending", 0) or 0) if engine is not None else 0
    if n:
        engine.reset_accumulation()
        if console is not None:
            console.print(f"    | gradient accumulation: dropped {n} micro-batch(es) of an unfinished cycle of {engine.grad_accum}")
    return n


# ---- revive_after (codebook revival): the codes a training stage restarted, in the trainers' logs ----------------------------------
def codes_revived_note(stats_stage_run: dict, stats_step: dict):
    """Add the step's revived-code count ("codes_revived_step": a device scalar of train_step's result, present only with the option
    on) to the stage's running sum.  Device arithmetic only: no synchronisation."""
    n = stats_step.get("codes_revived_step")
    if n is not None:
        stats_stage_run["codes_revived_run"] = stats_stage_run.get("codes_revived_run", 0) + n


def revive_epoch_record(engine, stats_stage_run: dict, stage: str = "train"):
    """End of a training stage, after its statistics were read: {"<stage>/codes_revived": codes restarted in this stage,
    "<stage>/codes_revived_total": so far in the run} | None with the option off."""
    total = stats_stage_run.pop("codes_revived_run", None)
    if engine is None or getattr(engine, "revive_after", None) is None or total is None:
        return None
    return {f"{stage}/codes_revived": int(total), f"{stage}/codes_revived_total": int(engine.revived_codes)}


# ---- TrainEngine(weight_ema=...): evaluation under the moving average of the weights, in the trainers ------------------------------
def weight_ema_scope(engine, enabled: bool = True):
    """The context a validation / test stage runs in: engine.weight_ema_applied() when the engine keeps an average and `enabled`
    (WEIGHT_EMA_EVAL) says to evaluate under it, a null context otherwise (no engine, option off, switched off)."""
    import contextlib
    if engine is None or getattr(engine, "weight_ema", None) is None or not enabled:
        return contextlib.nullcontext()
    return engine.weight_ema_applied()


def weight_ema_epoch_record(engine, last_decay=None, stage: str = "train"):
    """End of a training stage, after its statistics were read: {"<stage>/weight_ema_decay": the decay of the stage's last applied
    update (None before the first), "<stage>/weight_ema_updates": updates so far} | None with the option off."""
    if engine is None or getattr(engine, "weight_ema", None) is None:
        return None
    return {f"{stage}/weight_ema_decay": float(last_decay) if last_decay is not None else None,
            f"{stage}/weight_ema_updates": int(engine.weight_ema_updates)}


def param_groups_line(engine):
    """One line for the run's log with the engine's parameter-group table (pattern, lr scale, weight decay, parameter elements per
    group) | None without an engine or with param_groups / decoupled_weight_decay off."""
    if engine is None or getattr(engine, "_pg", None) is None:
        return None
    cells = [f"{g['group']}: {', '.join(g['match']) if g['match'] else '(everything else)'} lr x{g['lr_scale']:g} wd {g['weight_decay']:g} "
             f"{g['elements']} elements" for g in engine.param_group_table()]
    return f"parameter groups ({'decoupled' if engine.decoupled_wd else 'coupled'} weight decay) | " + " | ".join(cells)


def lr_epoch_record(engine, last_lr=None, stage: str = "train"):
    """End of a training stage, after its statistics were read: {"<stage>/lr": the learning rate of the stage's last optimiser step,
    from the device scalar the step handed out} | None without a learning-rate schedule (lr_warmup_steps / lr_decay)."""
    if engine is None or getattr(engine, "lr_schedule", None) is None or last_lr is None:
        return None
    return {f"{stage}/lr": float(last_lr)}
