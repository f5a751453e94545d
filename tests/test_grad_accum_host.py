"""Host-side checks of gradient accumulation (TrainEngine(grad_accum=A)): the option's validation needs no device, both entry-point
configurations carry GRAD_ACCUM_STEPS and honour KVQ_GRAD_ACCUM, include/kvq.h declares the two entry points and the ctypes table
knows them, every bad argument is refused before any HIP call, and the trainers count optimiser steps apart from calls."""
import importlib
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")
ENTRY_POINTS = ("kvq_grad_accumulate", "kvq_accum_advance")


def _config(model):
    sys.path.insert(0, os.path.join(PKG, "models", model))
    try:
        sys.modules.pop("config", None)
        return importlib.import_module("config")
    finally:
        sys.path.pop(0)
        sys.modules.pop("config", None)


def test_option_validation_needs_no_device(monkeypatch):
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    monkeypatch.delenv("KVQ_GRAD_ACCUM", raising=False)
    check = TrainEngine.check_grad_accum
    assert check(None) == 1 and check(None, env=True) == 1                      # unset: off
    assert check(1) == 1 and check(4) == 4 and check(4, env=True) == 4
    monkeypatch.setenv("KVQ_GRAD_ACCUM", "")
    assert check(None, env=True) == 1                                           # empty: off
    monkeypatch.setenv("KVQ_GRAD_ACCUM", "8")
    assert check(None, env=True) == 8 and check(None) == 1 and check(2, env=True) == 2
    for bad in (0, -1, 2.5, True, "x", "8", [2]):
        with pytest.raises(KvqError, match="grad_accum"):
            check(bad)
    for bad in ("0", "-1", "2.5", "x", "True"):
        monkeypatch.setenv("KVQ_GRAD_ACCUM", bad)
        with pytest.raises(KvqError, match="grad_accum"):
            check(None, env=True)


@pytest.mark.parametrize("model", ["shelgon3", "bagon"])
def test_config_carries_grad_accum_steps_and_honours_the_environment(model, monkeypatch):
    monkeypatch.delenv("KVQ_GRAD_ACCUM", raising=False)
    monkeypatch.delenv("KVQ_GRAD_ACCUM_STEPS", raising=False)
    cfg = _config(model)
    assert cfg.GRAD_ACCUM_STEPS == 1 and cfg.get_config()["grad_accum_steps"] == 1
    for text, want in (("8", 8), ("1", 1), ("", 1), (" 16 ", 16)):
        monkeypatch.setenv("KVQ_GRAD_ACCUM", text)
        cfg = _config(model)
        assert cfg.GRAD_ACCUM_STEPS == want and type(cfg.GRAD_ACCUM_STEPS) is int and cfg.get_config()["grad_accum_steps"] == want, text
    for bad in ("0", "-2", "2.5", "x", "True"):
        monkeypatch.setenv("KVQ_GRAD_ACCUM", bad)
        with pytest.raises(ValueError, match="GRAD_ACCUM_STEPS"):
            _config(model)
    monkeypatch.delenv("KVQ_GRAD_ACCUM")
    src = open(os.path.join(PKG, "models", model, "config.py")).read()
    line = next(l for l in src.splitlines() if l.startswith("GRAD_ACCUM_STEPS = 1"))
    assert "OPTIMISER steps" in line and "KVQ_GRAD_ACCUM" in line               # what the step counters count is said where the knob is
    main = open(os.path.join(PKG, "models", model, "main.py")).read()
    assert "grad_accum=GRAD_ACCUM_STEPS" in main and '"grad_accum"' in main     # handed to the engine, written to run_conf.json
    # the autograd path steps its optimiser on every batch: a run that asks for accumulation without the engine is refused, not
    # trained at another batch size in silence
    assert re.search(r"if engine is None and GRAD_ACCUM_STEPS > 1:.*\n\s+raise SystemExit\(.*GRAD_ACCUM_STEPS", main)
    trainer = open(os.path.join(PKG, "models", model, "Trainer.py")).read()
    assert "perf/optimizer_steps" in trainer and "perf/train_steps" in trainer and "drop_open_accumulation" in trainer


def test_header_declares_the_entry_points_and_the_ctypes_table_knows_them():
    from kvq import _ffi
    hdr = open(os.path.join(ROOT, "include", "kvq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _ffi.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
    assert "struct { uint64_t tick; uint32_t micro, pad; }" in hdr
    assert len(_ffi.SIGNATURES["kvq_grad_accumulate"][1]) == 7 and len(_ffi.SIGNATURES["kvq_accum_advance"][1]) == 3


def test_entry_points_refuse_before_any_launch():
    from kvq import _ffi
    lib = _ffi.lib()
    p = 4096                                                    # an aligned address that is never read: every call below is refused first
    assert lib.kvq_grad_accumulate(None, 16, 1, p, p, 2, None) == -1 and b"kvq_grad_accumulate" in lib.kvq_last_error()
    assert lib.kvq_grad_accumulate(p, 16, 1, None, p, 2, None) == -1 and b"null" in lib.kvq_last_error()
    assert lib.kvq_grad_accumulate(p, 16, 1, p, None, 2, None) == -1 and b"null" in lib.kvq_last_error()
    for n in (0, -8):
        assert lib.kvq_grad_accumulate(p, n, 1, p, p, 2, None) == -1 and b"n < 1" in lib.kvq_last_error()
    for A in (0, -1):
        assert lib.kvq_grad_accumulate(p, 16, 1, p, p, A, None) == -1 and b"A < 1" in lib.kvq_last_error()
    for dt in (2, -1, 7):
        assert lib.kvq_grad_accumulate(p, 16, dt, p, p, 2, None) == -1 and b"dtype" in lib.kvq_last_error()
    assert lib.kvq_grad_accumulate(p + 8, 16, 1, p, p, 2, None) == -1 and b"aligned" in lib.kvq_last_error()
    assert lib.kvq_grad_accumulate(p, 16, 0, p + 4, p, 2, None) == -1 and b"aligned" in lib.kvq_last_error()
    assert lib.kvq_accum_advance(None, 2, None) == -1 and b"kvq_accum_advance" in lib.kvq_last_error()
    for A in (0, -3):
        assert lib.kvq_accum_advance(p, A, None) == -1 and b"A < 1" in lib.kvq_last_error()
    assert lib.kvq_accum_advance(p + 4, 2, None) == -1 and b"aligned" in lib.kvq_last_error()


def test_wrappers_refuse_what_is_not_an_accumulation_state():
    import torch
    from kvq import nnops
    from kvq._ffi import KvqError
    for bad in (None, torch.zeros(2, dtype=torch.int64), torch.zeros(4, dtype=torch.float32)):      # a CPU tensor is no state
        with pytest.raises(KvqError):
            nnops.read_accum_state(bad)
        with pytest.raises(KvqError):
            nnops.accum_advance(bad, 2)


def test_flat_accumulator_is_lazy():
    """FlatParams.acc exists only once somebody asks for it: an engine without the option never allocates it."""
    import torch
    from kvq.engine import FlatParams
    P = lambda *shape: torch.nn.Parameter(torch.randn(*shape))
    fl = FlatParams([("a", P(4, 16), 64), ("odd", P(9), 9)], "cpu", torch.bfloat16, amsgrad=False)
    assert fl._acc is None and not fl.optimizer_state_allocated()
    assert fl.acc.dtype == torch.float32 and fl.acc.numel() == fl.n and fl.acc is fl.acc and fl._grad is None


def test_runlog_counts_optimizer_steps_and_averages_the_norm_over_them():
    import torch
    from kvq.runlog import grad_guard_epoch_record, grad_norm_note, optimizer_step_note, optimizer_steps_epoch

    class Eng:
        max_grad_norm, skipped_steps = 1.0, 0

    run = {}
    for i in range(7):                                           # A = 3: calls 3 and 6 ran the optimiser, call 7 opens a cycle
        final = i % 3 == 2
        stats = {"optimizer_step": final}
        if final:
            stats["grad_norm_step"] = torch.tensor(2.0 if i == 2 else 4.0)
        grad_norm_note(run, stats)
        optimizer_step_note(run, stats)
    optimizer_step_note(run, {"loss_recon_step": torch.tensor(1.0)})            # a step without the key is not counted
    rec, skipped = grad_guard_epoch_record(Eng(), run, n_steps=7, skipped_before=0)
    assert rec == {"train/grad_norm": 3.0, "train/skipped_steps": 0} and skipped == 0      # (2 + 4) / 2 optimiser steps, not / 7 calls
    assert optimizer_steps_epoch(run, 7) == 2 and "optimizer_steps_run" not in run
    assert optimizer_steps_epoch({}, 7) == 7                                    # no step carried the key: every call was a step


class _StubEngine:
    """What the trainers see of a TrainEngine(grad_accum=A, max_grad_norm=inf): train_step / eval_step results and the bookkeeping
    members."""

    def __init__(self, A):
        import torch
        self.grad_accum, self.max_grad_norm, self.skipped_steps = A, float("inf"), 0
        self.accum_pending = self.calls = self.resets = 0
        self._t = torch

    def _out(self, ids):
        t = self._t
        return dict(loss_recon=t.tensor(1.0), loss_vq=t.tensor(0.5), perplexity=t.tensor(3.0), acc=t.tensor(0.25), recon_ids=ids,
                    acc_per_sentence=t.full((ids.shape[0],), 0.25))

    def train_step(self, ids, mask, prepared=None, **kw):
        self.calls += 1
        out = self._out(ids)
        final = self.accum_pending == self.grad_accum - 1
        self.accum_pending = 0 if final else self.accum_pending + 1
        out["optimizer_step"] = final
        if final:
            out["grad_norm"] = self._t.tensor(float(self.calls))
        return out

    def eval_step(self, ids, mask, **kw):
        return self._out(ids)

    def reset_accumulation(self):
        self.resets += 1
        self.accum_pending = 0


class _Log:
    def __init__(self):
        self.lines = []

    def log(self, d):
        self.lines.append(d)

    def print(self, s):
        self.lines.append(s)


class _Model:
    def train(self):
        return self

    def eval(self):
        return self


def _batches(n):
    import torch
    return [dict(input_ids=torch.ones(4, 6, dtype=torch.int64), attention_mask=torch.ones(4, 6, dtype=torch.int64)) for _ in range(n)]


def test_shelgon_trainer_counts_optimizer_steps_and_drops_an_open_cycle():
    """Five batches per epoch at A = 3: epoch 1 makes one optimiser step and leaves two micro-batches pending, which carry into epoch
    2 (two steps there, after calls 6 and 9); validation does not touch the cycle; the one micro-batch open at the end is dropped
    with one console line."""
    from models.shelgon3 import Trainer as T
    eng, wandb, console = _StubEngine(3), _Log(), _Log()
    T.train(None, console, "cpu", _batches(5), _batches(2), 5, 2, _Model(), None, False, 100, [], object(), 1.0, 1.0, 1.0, 1.0, 1.0, 0.0,
            None, 2, 1000, wandb, "unused", False, engine=eng)
    perf = [d for d in wandb.lines if "perf/train_steps" in d]
    assert [(d["perf/train_steps"], d["perf/optimizer_steps"]) for d in perf] == [(5, 1), (5, 2)]
    norms = [d["train/grad_norm"] for d in wandb.lines if "train/grad_norm" in d]
    assert norms == [3.0, (6.0 + 9.0) / 2]                         # the stub's norm is the call number: averaged over optimiser steps
    assert eng.calls == 10 and eng.resets == 1 and eng.accum_pending == 0
    dropped = [s for s in console.lines if isinstance(s, str) and "gradient accumulation" in s]
    assert len(dropped) == 1 and "dropped 1 " in dropped[0]


def test_bagon_trainer_counts_optimizer_steps_and_drops_an_open_cycle():
    from models.bagon import Trainer as T
    eng, wandb, console = _StubEngine(2), _Log(), _Log()
    T.train(None, console, "cpu", _batches(3), _batches(1), 3, 1, _Model(), None, None, False, 6, False, 6, 0.0, 0.0, 0.0, 0.0,
            100, [], object(), None, 1, 1000, 1000, wandb, "unused", export_checkpoint=False, engine=eng)
    perf = [d for d in wandb.lines if "perf/train_steps" in d]
    assert [(d["perf/train_steps"], d["perf/optimizer_steps"]) for d in perf] == [(3, 1)]
    assert [d["train/grad_norm"] for d in wandb.lines if "train/grad_norm" in d] == [2.0]
    assert eng.resets == 1 and sum("gradient accumulation" in s for s in console.lines if isinstance(s, str)) == 1


def test_an_engine_without_the_option_leaves_the_trainers_as_they_were():
    """No engine / grad_accum 1 with nothing pending: no console line, nothing reset."""
    from kvq.runlog import drop_open_accumulation
    console = _Log()
    assert drop_open_accumulation(None, console) == 0
    eng = _StubEngine(1)
    assert drop_open_accumulation(eng, console) == 0 and eng.resets == 0 and console.lines == []
