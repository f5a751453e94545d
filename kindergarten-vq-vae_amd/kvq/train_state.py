"""One training-state file per run: what a killed run needs to continue at the next epoch, bit for bit on the engine path
(DESIGN.md section 5e).  Shared by models/shelgon3 and models/bagon.

The file is a dict: `format`, `model_state_dict` (complete, the reference's keys: the file reads like a best-val checkpoint),
`engine` (TrainEngine.state_dict()) -- or, on the autograd path, `optimizer` and `lr_scheduler` --, `trainer` (last finished
epoch, best statistics, history, counters, decoded sentences, the train loader's epoch), `rng` (torch's CPU and device
generators: the DataLoader shuffle draws from the first, Bagon's token noise from the second) and `config`.  Plain data only: it
loads with torch.load(weights_only=True).

Rank 0 writes, atomically (`<name>.tmp`, then os.replace), and a barrier follows the write; every rank reads the same file, so a
multi-rank run needs a filesystem all ranks share (kvq.ddp.readable_everywhere stops all ranks together when one cannot read
it).  Resume is at epoch granularity."""
from __future__ import annotations

import os

import torch

TRAIN_STATE_FORMAT = 1
# what decides WHICH batches an epoch holds (everything numeric is the engine fingerprint's business): compared on resume
RESUME_CONFIG_KEYS = ("batch_size", "train_split_pct", "val_split_pct", "ds_gen_seed", "token_cache", "tokenized_sentence_max_length",
                      "world_size")


class TrainStateError(RuntimeError):
    pass


def _plain(obj):
    """obj as plain data: CPU tensors, Python scalars / strings / None, lists and dicts with string keys (tuples become lists,
    numpy and 0-d tensor scalars Python numbers) -- what torch.load(weights_only=True) accepts."""
    if torch.is_tensor(obj):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        return {(k if isinstance(k, (str, int)) else str(k)): _plain(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_plain(v) for v in obj]
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    if hasattr(obj, "item") and getattr(obj, "shape", None) == ():           # numpy scalars
        return obj.item()
    raise TrainStateError(f"train state: cannot store a {type(obj).__name__} as plain data")


def check_every(v, name="TRAIN_STATE_EVERY_EPOCHS"):
    """The integer >= 1 TRAIN_STATE_EVERY_EPOCHS / train(train_state_every=...) accepts; anything else raises ValueError."""
    if isinstance(v, bool) or not isinstance(v, int) or v < 1:
        raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    return v


def trainer_state(epoch, stats_train_best, stats_val_best, history, skipped, decoded_sentences, dl_train) -> dict:
    """The `trainer` entry: what train() itself carries from one epoch to the next."""
    return {"epoch": int(epoch), "stats_train_best": dict(stats_train_best), "stats_val_best": dict(stats_val_best),
            "history": [[dict(t), dict(v)] for t, v in history], "skipped": int(skipped), "decoded_sentences": list(decoded_sentences),
            "loader_epoch": int(dl_train.epoch) if isinstance(getattr(dl_train, "epoch", None), int) else None}


def rng_state() -> dict:
    return {"cpu": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state() if torch.cuda.is_available() else None}


def restore_rng(rng: dict) -> None:
    torch.set_rng_state(rng["cpu"].cpu())
    if rng.get("cuda") is not None and torch.cuda.is_available():
        torch.cuda.set_rng_state(rng["cuda"].cpu())


def restore_trainer(resume: dict, decoded_sentences: list, dl_train):
    """(first epoch to run, stats_train_best, stats_val_best, history, skipped) of a resumed train(); decoded_sentences is
    refilled in place, the train loader's epoch counter and the generators are set to where the stored run stood."""
    tr = resume["trainer"]
    decoded_sentences[:] = list(tr["decoded_sentences"])
    if tr.get("loader_epoch") is not None and hasattr(dl_train, "epoch"):
        dl_train.epoch = int(tr["loader_epoch"])
    restore_rng(resume["rng"])
    history = [(dict(t), dict(v)) for t, v in tr["history"]]
    return int(tr["epoch"]) + 1, dict(tr["stats_train_best"]), dict(tr["stats_val_best"]), history, int(tr["skipped"])


def save_train_state(path, model, trainer: dict, config: dict, engine=None, opt=None, lr_sched=None, is_main: bool = True) -> None:
    """Write the run's training state to `path`.  Every rank calls it: rank 0 (`is_main`) gathers and writes, the others wait at
    the barrier behind the write.  Atomic: a write that fails leaves the previous file as it was."""
    import torch.distributed as dist
    try:
        if is_main:
            state = {"format": TRAIN_STATE_FORMAT, "model_state_dict": _plain(model.state_dict()), "trainer": _plain(trainer),
                     "rng": rng_state(), "config": _plain(config)}
            if engine is not None:
                state["engine"] = engine.state_dict()
            else:
                state["optimizer"] = _plain(opt.state_dict()) if opt is not None else None
                state["lr_scheduler"] = _plain(lr_sched.state_dict()) if lr_sched is not None else None
            tmp = str(path) + ".tmp"
            try:
                torch.save(state, tmp)
                os.replace(tmp, path)
            except BaseException:
                if os.path.exists(tmp):
                    os.remove(tmp)
                raise
    finally:
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.barrier()


def load_train_state(path, map_location="cpu") -> dict:
    """The dict save_train_state wrote (plain data: weights_only=True).  The engine's entry holds CPU tensors whatever
    map_location says for the rest: TrainEngine.load_state_dict copies them into its own buffers."""
    state = torch.load(path, map_location=map_location, weights_only=True)
    if not isinstance(state, dict) or state.get("format") != TRAIN_STATE_FORMAT:
        got = state.get("format") if isinstance(state, dict) else type(state).__name__
        raise TrainStateError(f"{path}: not a training-state file of format {TRAIN_STATE_FORMAT} (format: {got!r})")
    missing = [k for k in ("model_state_dict", "trainer", "rng", "config") if k not in state] + \
        ([] if "engine" in state or "optimizer" in state else ["engine | optimizer"])
    if missing:
        raise TrainStateError(f"{path}: training-state file without {', '.join(missing)}")
    return state


def resolve_path(resume_from, file_name: str) -> str:
    """RESUME_FROM is a run directory or a state file: the state file's path."""
    resume_from = str(resume_from)
    return os.path.join(resume_from, file_name) if os.path.isdir(resume_from) else resume_from


def config_differences(stored: dict, current: dict, keys=RESUME_CONFIG_KEYS) -> list:
    """["key: stored a, now b", ...] for exactly the keys of `keys` whose values differ (a key one side lacks differs)."""
    miss = object()
    out = []
    for k in keys:
        a, b = stored.get(k, miss), current.get(k, miss)
        if a is miss and b is miss:
            continue
        if a is miss or b is miss or a != b:
            out.append(f"{k}: stored {'(absent)' if a is miss else repr(a)}, now {'(absent)' if b is miss else repr(b)}")
    return out


def load_optimizer(state: dict, opt, lr_sched) -> None:
    """The autograd path: torch's own optimiser / scheduler state."""
    if state.get("optimizer") is not None and opt is not None:
        opt.load_state_dict(state["optimizer"])
    if state.get("lr_scheduler") is not None and lr_sched is not None:
        # (milestones: a collections.Counter in torch's dict, a plain dict in the file; the scheduler at hand was built from the
        #  configuration's and keeps its own)
        lr_sched.load_state_dict({k: v for k, v in state["lr_scheduler"].items() if k != "milestones"})
