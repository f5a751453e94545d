"""Host-side checks of the weight EMA (TrainEngine(weight_ema=decay)): the numpy restatement of the kernels
against hand-computed values, the option's validation (no device needed), both entry-point configurations, the header and the
ctypes table, refusals before any HIP call, the training-state helpers on a state with the new entries, and the trainers' use of
the evaluation scope."""
import contextlib
import importlib
import os
import re
import sys

import numpy as np
import pytest

import _weight_ema_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")
ENTRY_POINTS = ("kvq_weight_ema_update", "kvq_weight_ema_advance", "kvq_weight_ema_swap")
f32, f64 = np.float32, np.float64


def _config(model):
    sys.path.insert(0, os.path.join(PKG, "models", model))
    try:
        sys.modules.pop("config", None)
        return importlib.import_module("config")
    finally:
        sys.path.pop(0)
        sys.modules.pop("config", None)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def test_decay_schedule_by_hand():
    assert R.decay_at(1, 0.999) == f64(2.0) / f64(11.0)                      # (1 + 1) / (10 + 1)
    assert R.decay_at(5, 0.999) == f64(6.0) / f64(15.0) == f64(0.4)
    assert R.decay_at(10 ** 6, 0.999) == f64(f32(0.999))                     # a large t caps d at the decay -- the FLOAT the call takes
    assert R.decay_at(10 ** 6, 0.999) != f64(0.999)
    # decay 0.9: (1 + t) / (10 + t) reaches 0.9 at t = 80 (81 / 90); float(0.9) lies just below 0.9 and wins there
    assert R.decay_at(79, 0.9) == f64(80.0) / f64(89.0) < f64(f32(0.9))
    assert R.decay_at(80, 0.9) == f64(f32(0.9)) < f64(81.0) / f64(90.0)
    assert R.decay_at(2 ** 40, 0.5) == f64(0.5)


def test_update_by_hand():
    # t = 5: d = 0.4; 0.4 * 2 = 0.8, (1 - 0.4) * 4 = 2.4, 0.8 + 2.4 = 3.2 in f64, rounded once to f32
    got = R.update(f32([4.0]), f32([2.0]), 5, 0.999)
    assert got.dtype == np.float32 and got[0] == f32(f64(0.4) * f64(2.0) + (f64(1.0) - f64(0.4)) * f64(4.0)) == f32(3.2)
    # t = 1: d = 2/11; ema 0, p 1 -> 1 - 2/11
    assert R.update(f32([1.0]), f32([0.0]), 1, 0.999)[0] == f32(f64(1.0) - f64(2.0) / f64(11.0))
    # a weight that does not move keeps its average EXACTLY: 1 - d is exact for d in [0.5, 1] and d + (1 - d) = 1 -- in f32
    # arithmetic, with 1 - float(0.9999) rounded, it would creep
    ones = np.ones(5, dtype=np.float32)
    assert np.array_equal(R.update(ones, ones, 10 ** 6, 0.9999), ones)
    # the products are rounded before the sum (no FMA): d * ema alone needs more than 53 bits here
    e, p, d = f32(1.0000001), f32(3.0000002), R.decay_at(10 ** 6, 0.999)
    assert R.update(f32([p]), f32([e]), 10 ** 6, 0.999)[0] == f32(d * f64(e) + (f64(1.0) - d) * f64(p))


def test_first_update_stores_and_skip_keeps():
    p = f32([1.5, -0.0, 3e-40])
    nan = np.full(3, np.nan, dtype=np.float32)
    assert R.same_bits(R.update(p, nan, 0, 0.999), p).size == 0              # ema is not read: the NaN does not survive
    assert R.same_bits(R.update(p, None, 0, 0.999), p).size == 0
    assert np.isnan(R.update(p, nan, 1, 0.999)).all()                        # later updates do read it
    old = f32([7.0, 8.0, 9.0])
    for t in (0, 1, 10 ** 6):
        assert R.same_bits(R.update(p, old, t, 0.999, skip=True), old).size == 0
    assert R.advance((4, 0.25), 0.999, skip=True) == (4, 0.25)


def test_advance_by_hand():
    s = (0, 0.0)
    s = R.advance(s, 0.999)
    assert s == (1, 0.0)                                                     # the storing step reports 0
    s = R.advance(s, 0.999)
    assert s == (2, float(f32(f64(2.0) / f64(11.0))))
    s = R.advance(s, 0.999)
    assert s == (3, float(f32(f64(3.0) / f64(12.0)))) == (3, 0.25)
    assert R.advance((10 ** 6, 0.0), 0.999) == (10 ** 6 + 1, float(f32(0.999)))


def test_special_operands_follow_ieee():
    inf, big, den = f32(np.inf), np.finfo(np.float32).max, f32(1e-45)
    up = lambda p, e: R.update(f32([p]), f32([e]), 5, 0.999)[0]
    assert up(inf, 1.0) == inf and up(1.0, -inf) == -inf and np.isnan(up(inf, -inf)) and np.isnan(up(np.nan, 1.0))
    assert up(big, big) == big and up(-big, -big) == -big                    # 0.4 max + 0.6 max rounds back to max, no overflow
    assert up(den, den) == den                                               # denormals are neither flushed on the way in nor out
    assert np.signbit(up(-0.0, -0.0)) and not np.signbit(up(0.0, -0.0))


def test_bf16_rounding_and_swap():
    x = f32([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -2.5, np.inf, 0.0, -0.0, 3.0e38])
    assert R.bf16_bits(x).tolist() == [0x3F80, 0x3F80, 0x3F82, 0xC020, 0x7F80, 0x0000, 0x8000, 0x7F62]      # ties go to even
    assert R.same_bits_bf16(R.bf16_bits(f32([np.nan])), np.uint16([0xFFC1])).size == 0
    assert R.same_bits_bf16(np.uint16([0x7F80]), np.uint16([0x7FC0])).tolist() == [0]                        # inf is no NaN
    p, e = f32([1.0, 2.0, np.nan]), f32([3.0, -0.0, 5.0])
    p2, e2, sh = R.swap(p, e, shadow=True)
    assert R.same_bits(p2, e).size == 0 and R.same_bits(e2, p).size == 0 and sh.tolist() == [0x4040, 0x8000, 0x40A0]
    p3, e3, none = R.swap(p2, e2)
    assert none is None and R.same_bits(p3, p).size == 0 and R.same_bits(e3, e).size == 0
    assert R.same_bits(f32([1.0, np.nan]), f32([1.0, -np.nan])).size == 0 and R.same_bits(f32([0.0]), f32([-0.0])).tolist() == [0]


# ---- the option --------------------------------------------------------------------------------------------------------------------
def test_option_validation_needs_no_device(monkeypatch):
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    monkeypatch.delenv("KVQ_WEIGHT_EMA", raising=False)
    check = TrainEngine.check_weight_ema
    assert check(None) is None and check(None, env=True) is None                # unset: off
    assert check(0.999) == 0.999 and check(0.5, env=True) == 0.5 and type(check(0.5)) is float
    monkeypatch.setenv("KVQ_WEIGHT_EMA", "")
    assert check(None, env=True) is None                                        # empty: off
    monkeypatch.setenv("KVQ_WEIGHT_EMA", "0.9999")
    assert check(None, env=True) == 0.9999 and check(None) is None and check(0.9, env=True) == 0.9
    for bad in (0, 1, 0.0, 1.0, -0.5, 1.5, True, False, "0.9", [0.9], float("nan"), float("inf")):
        with pytest.raises(KvqError, match="weight_ema"):
            check(bad)
    for bad in ("0", "1", "-0.5", "2", "x", "True", "nan", "inf"):
        monkeypatch.setenv("KVQ_WEIGHT_EMA", bad)
        with pytest.raises(KvqError, match="weight_ema"):
            check(None, env=True)


@pytest.mark.parametrize("model", ["shelgon3", "bagon"])
def test_config_carries_the_decay_and_honours_the_environment(model, monkeypatch):
    for k in ("KVQ_WEIGHT_EMA", "KVQ_WEIGHT_EMA_DECAY", "KVQ_WEIGHT_EMA_EVAL"):
        monkeypatch.delenv(k, raising=False)
    cfg = _config(model)
    assert cfg.WEIGHT_EMA_DECAY is None and cfg.WEIGHT_EMA_EVAL is True
    assert cfg.get_config()["weight_ema_decay"] is None and cfg.get_config()["weight_ema_eval"] is True
    for text, want in (("0.999", 0.999), ("", None), (" 0.5 ", 0.5)):
        monkeypatch.setenv("KVQ_WEIGHT_EMA", text)
        assert _config(model).WEIGHT_EMA_DECAY == want, text
    for bad in ("0", "1", "1.5", "-0.1", "x", "True"):
        monkeypatch.setenv("KVQ_WEIGHT_EMA", bad)
        with pytest.raises(ValueError, match="WEIGHT_EMA_DECAY"):
            _config(model)
    monkeypatch.delenv("KVQ_WEIGHT_EMA")
    monkeypatch.setenv("KVQ_WEIGHT_EMA_EVAL", "False")
    assert _config(model).WEIGHT_EMA_EVAL is False
    monkeypatch.setenv("KVQ_WEIGHT_EMA_EVAL", "maybe")
    with pytest.raises(ValueError, match="WEIGHT_EMA_EVAL"):
        _config(model)
    monkeypatch.delenv("KVQ_WEIGHT_EMA_EVAL")
    main = open(os.path.join(PKG, "models", model, "main.py")).read()
    assert "weight_ema=WEIGHT_EMA_DECAY" in main and "weight_ema_eval=WEIGHT_EMA_EVAL" in main and '"weight_ema"' in main
    # the average is built inside the engine's step: a run that asks for it without the engine is refused
    assert re.search(r"if engine is None and WEIGHT_EMA_DECAY is not None:.*\n\s+raise SystemExit\(.*WEIGHT_EMA_DECAY", main)


def test_header_declares_the_entry_points_and_the_ctypes_table_knows_them():
    from kvq import _ffi
    hdr = open(os.path.join(ROOT, "include", "kvq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _ffi.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
    assert "struct { uint64_t updates; float last_decay; uint32_t pad; }" in hdr
    assert [len(_ffi.SIGNATURES[n][1]) for n in ENTRY_POINTS] == [7, 4, 5]


def test_entry_points_refuse_before_any_launch():
    from kvq import _ffi
    lib = _ffi.lib()
    p, q = 4096, 1 << 20                                        # aligned, disjoint addresses that are never read: every call is refused first
    err = lambda: lib.kvq_last_error()
    for args in ((None, q, 16, 0.9, p, None, None), (p, None, 16, 0.9, p, None, None), (p, q, 16, 0.9, None, None, None)):
        assert lib.kvq_weight_ema_update(*args) == -1 and b"kvq_weight_ema_update" in err() and b"null" in err()
    for n in (0, -4):
        assert lib.kvq_weight_ema_update(p, q, n, 0.9, p, None, None) == -1 and b"n < 1" in err()
    for d in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert lib.kvq_weight_ema_update(p, q, 16, d, p, None, None) == -1 and b"decay" in err()
        assert lib.kvq_weight_ema_advance(p, d, None, None) == -1 and b"kvq_weight_ema_advance" in err() and b"decay" in err()
    for args in ((p + 4, q, 16, 0.9, p, None, None), (p, q + 8, 16, 0.9, p, None, None), (p, q, 16, 0.9, p + 4, None, None),
                 (p, q, 16, 0.9, p, p + 4, None)):
        assert lib.kvq_weight_ema_update(*args) == -1 and b"aligned" in err()
    assert lib.kvq_weight_ema_update(p, p + 32, 16, 0.9, q, None, None) == -1 and b"overlap" in err()
    assert lib.kvq_weight_ema_advance(None, 0.9, None, None) == -1 and b"null" in err()
    assert lib.kvq_weight_ema_advance(p + 4, 0.9, None, None) == -1 and b"aligned" in err()
    assert lib.kvq_weight_ema_advance(p, 0.9, p + 4, None) == -1 and b"aligned" in err()
    for args in ((None, q, None, 16, None), (p, None, None, 16, None)):
        assert lib.kvq_weight_ema_swap(*args) == -1 and b"kvq_weight_ema_swap" in err() and b"null" in err()
    assert lib.kvq_weight_ema_swap(p, q, None, 0, None) == -1 and b"n < 1" in err()
    assert lib.kvq_weight_ema_swap(p + 8, q, None, 16, None) == -1 and b"aligned" in err()
    assert lib.kvq_weight_ema_swap(p, q, p + 4, 16, None) == -1 and b"aligned" in err()
    assert lib.kvq_weight_ema_swap(p, p, None, 16, None) == -1 and b"overlap" in err()                  # p == ema
    assert lib.kvq_weight_ema_swap(p, p + 48, None, 16, None) == -1 and b"overlap" in err()             # 16 floats = 64 bytes
    assert lib.kvq_weight_ema_swap(p, q, q + 32, 16, None) == -1 and b"shadow" in err()


def test_wrappers_refuse_what_is_not_a_weight_ema_state():
    import torch
    from kvq import nnops
    from kvq._ffi import KvqError
    for bad in (None, torch.zeros(2, dtype=torch.int64), torch.zeros(4, dtype=torch.float32)):      # a CPU tensor is no state
        with pytest.raises(KvqError):
            nnops.read_weight_ema_state(bad)
        with pytest.raises(KvqError):
            nnops.weight_ema_advance(bad, 0.9)


def test_flat_average_is_lazy():
    """FlatParams.ema exists only once somebody asks for it: an engine without the option never allocates it."""
    import torch
    from kvq.engine import FlatParams
    P = lambda *shape: torch.nn.Parameter(torch.randn(*shape))
    fl = FlatParams([("a", P(4, 16), 64), ("odd", P(9), 9)], "cpu", torch.bfloat16, amsgrad=False)
    assert fl._ema is None and not fl.optimizer_state_allocated()
    assert fl.ema.dtype == torch.float32 and fl.ema.numel() == fl.n and fl.ema is fl.ema and fl._grad is None and fl._acc is None


# ---- training state -----------------------------------------------------------------------------------------------------------------
def test_train_state_helpers_accept_a_state_with_the_new_entries(tmp_path):
    """The engine's state with the option on -- fingerprint.weight_ema, flat.ema, aux.i.ema, structs.weight_ema -- is plain data:
    it goes through save_train_state / load_train_state (torch.load(weights_only=True)) unchanged."""
    import torch
    from kvq.train_state import _plain, load_train_state, save_train_state, trainer_state
    wema = torch.tensor([7, int(np.float32(0.4).view(np.uint32))], dtype=torch.int64)
    eng_state = {"format": 1, "kvq_version": 100, "fingerprint": {"flat_n": 32, "weight_ema": 0.999},
                 "flat": {"master": torch.randn(32), "ema": torch.randn(32)},
                 "aux": [{"p": torch.randn(4, 8), "m": torch.zeros(4, 8), "v": torch.zeros(4, 8), "ema": torch.randn(4, 8)}],
                 "structs": {"state": torch.zeros(3, dtype=torch.int64), "weight_ema": wema},
                 "host": {"step": 7, "accum_pending": 0, "grads_are_mean": False}}
    assert _plain(eng_state)["fingerprint"]["weight_ema"] == 0.999

    class Eng:
        def state_dict(self):
            return eng_state

    class Loader:
        epoch = 3

    path = str(tmp_path / "state.pth")
    model = torch.nn.Linear(2, 2)
    save_train_state(path, model, trainer_state(3, {"a_best": 1.0}, {"a_best": 2.0}, [], 0, [], Loader()), {"batch_size": 4}, engine=Eng())
    back = load_train_state(path)["engine"]
    assert back["fingerprint"] == eng_state["fingerprint"] and back["host"] == eng_state["host"]
    assert torch.equal(back["flat"]["ema"], eng_state["flat"]["ema"]) and torch.equal(back["aux"][0]["ema"], eng_state["aux"][0]["ema"])
    assert torch.equal(back["structs"]["weight_ema"], wema)
    assert float(back["structs"]["weight_ema"][1:2].view(torch.float32)[0]) == float(np.float32(0.4))


# ---- the trainers -------------------------------------------------------------------------------------------------------------------
class _StubEngine:
    """What the trainers see of a TrainEngine(weight_ema=d): results of train_step / eval_step, the scope, the update count; every
    call is filed with whether the scope was open."""

    def __init__(self, decay):
        import torch
        self._t, self.weight_ema, self.weight_ema_updates, self.applied, self.events = torch, decay, 0, False, []
        self.grad_accum, self.max_grad_norm, self.accum_pending = 1, None, 0

    def _out(self, ids):
        t = self._t
        return dict(loss_recon=t.tensor(1.0), loss_vq=t.tensor(0.5), perplexity=t.tensor(3.0), acc=t.tensor(0.25), recon_ids=ids,
                    acc_per_sentence=t.full((ids.shape[0],), 0.25))

    def train_step(self, ids, mask, prepared=None, **kw):
        assert not self.applied, "train_step inside the scope"
        self.events.append(("train", self.applied))
        out = self._out(ids)
        out["optimizer_step"] = True
        if self.weight_ema is not None:
            t = self.weight_ema_updates
            out["weight_ema_decay"] = self._t.tensor(0.0 if t == 0 else min(self.weight_ema, (1 + t) / (10 + t)))
            self.weight_ema_updates += 1
        return out

    def eval_step(self, ids, mask, **kw):
        self.events.append(("eval", self.applied))
        return self._out(ids)

    @contextlib.contextmanager
    def weight_ema_applied(self):
        assert self.weight_ema is not None and not self.applied
        self.applied = True
        self.events.append(("enter", True))
        try:
            yield self
        finally:
            self.applied = False
            self.events.append(("exit", False))

    def state_dict(self):
        assert not self.applied, "state_dict inside the scope"
        self.events.append(("state_dict", self.applied))
        return {}


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

    def state_dict(self):
        return {}


class _Tok:
    def batch_decode(self, sequences):
        return ["s"] * len(sequences)


def _batches(n):
    import torch
    return [dict(input_ids=torch.ones(4, 6, dtype=torch.int64), attention_mask=torch.ones(4, 6, dtype=torch.int64)) for _ in range(n)]


def _shelgon_train(eng, wandb, console, tmp_path, monkeypatch, **kw):
    from models.shelgon3 import Trainer as T
    monkeypatch.setattr(T, "checkpoint", lambda best, model, d, stage: eng.events.append(("checkpoint_" + stage, eng.applied)))
    T.train(None, console, "cpu", _batches(3), _batches(2), 3, 2, _Model(), None, False, 100, [], object(), 1.0, 1.0, 1.0, 1.0, 1.0, 0.0,
            None, 2, 1000, wandb, str(tmp_path), True, engine=eng, train_state_path=str(tmp_path / "s.pth"), **kw)
    return T


def test_shelgon_trainer_validates_and_checkpoints_under_the_average(tmp_path, monkeypatch):
    eng, wandb, console = _StubEngine(0.999), _Log(), _Log()
    T = _shelgon_train(eng, wandb, console, tmp_path, monkeypatch)
    epoch = [("train", False)] * 3 + [("enter", True)] + [("eval", True)] * 2 + [("checkpoint_val", True), ("exit", False),
                                                                                ("state_dict", False)]
    assert eng.events == epoch * 2, eng.events            # validation and the best-val checkpoint inside, save_train_state outside
    recs = [d for d in wandb.lines if isinstance(d, dict) and "train/weight_ema_updates" in d]
    assert [(d["train/weight_ema_updates"], d["train/weight_ema_decay"]) for d in recs] == \
        [(3, pytest.approx(3 / 12)), (6, pytest.approx(6 / 15))]
    lines = [s for s in console.lines if isinstance(s, str) and "weight EMA" in s]
    assert len(lines) == 2 and "updates: 3" in lines[0] and "updates: 6" in lines[1]          # one console line per epoch
    eng.events.clear()
    T.test(None, console, "cpu", _batches(2), 2, _Model(), _Tok(), False, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, [], 1000, 2, wandb, engine=eng)
    assert eng.events == [("enter", True), ("eval", True), ("eval", True), ("exit", False)]
    eng.events.clear()
    T.test(None, console, "cpu", _batches(1), 1, _Model(), _Tok(), False, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, [], 1000, 2, wandb, engine=eng,
           weight_ema_eval=False)
    assert eng.events == [("eval", False)]


def test_shelgon_trainer_with_evaluation_under_the_average_switched_off(tmp_path, monkeypatch):
    eng, wandb, console = _StubEngine(0.999), _Log(), _Log()
    _shelgon_train(eng, wandb, console, tmp_path, monkeypatch, weight_ema_eval=False)
    assert ("enter", True) not in eng.events and ("eval", False) in eng.events and ("checkpoint_val", False) in eng.events
    assert sum("weight EMA" in s and "live weights" in s for s in console.lines if isinstance(s, str)) == 2


def test_bagon_trainer_validates_and_checkpoints_under_the_average(tmp_path, monkeypatch):
    from models.bagon import Trainer as T
    eng, wandb, console = _StubEngine(0.9), _Log(), _Log()
    monkeypatch.setattr(T, "checkpoint", lambda best, model, d, stage: eng.events.append(("checkpoint_" + stage, eng.applied)))
    T.train(None, console, "cpu", _batches(2), _batches(1), 2, 1, _Model(), None, None, False, 6, False, 6, 0.0, 0.0, 0.0, 0.0,
            100, [], object(), None, 1, 1000, 1000, wandb, str(tmp_path), export_checkpoint=True, engine=eng,
            train_state_path=str(tmp_path / "s.pth"))
    assert eng.events == [("train", False), ("train", False), ("checkpoint_train", False), ("enter", True), ("eval", True),
                          ("checkpoint_val", True), ("exit", False), ("state_dict", False)], eng.events
    assert sum("weight EMA" in s for s in console.lines if isinstance(s, str)) == 1
    eng.events.clear()
    T.test(None, console, "cpu", _batches(1), 1, _Model(), _Tok(), _Tok(), False, 6, False, 6, 0.0, 0.0, [], 1000, 1000, 1, wandb, engine=eng)
    assert eng.events == [("enter", True), ("eval", True), ("exit", False)]


def test_an_engine_without_the_option_leaves_the_trainers_as_they_were(tmp_path, monkeypatch):
    """Option off (or no engine): no scope, no log record, no console line."""
    from kvq.runlog import weight_ema_epoch_record, weight_ema_scope
    eng, wandb, console = _StubEngine(None), _Log(), _Log()
    _shelgon_train(eng, wandb, console, tmp_path, monkeypatch)
    assert ("enter", True) not in eng.events and ("eval", False) in eng.events
    assert not any("weight EMA" in s for s in console.lines if isinstance(s, str))
    assert not any("train/weight_ema_updates" in d for d in wandb.lines if isinstance(d, dict))
    assert weight_ema_epoch_record(None) is None and weight_ema_epoch_record(eng) is None
    with weight_ema_scope(None), weight_ema_scope(eng), weight_ema_scope(_StubEngine(0.9), enabled=False):
        pass
