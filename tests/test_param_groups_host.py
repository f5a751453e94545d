"""Host-side checks of the parameter groups, the decoupled decay switch and the learning-rate schedule options:
pattern resolution, the block-table builder on a synthetic FlatParams-shaped layout, the options' validation and environment
parsing (no device needed), both entry-point configurations and both main.py."""
import importlib
import json
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")
ENV = ("KVQ_PARAM_GROUPS", "KVQ_DECOUPLED_WD", "KVQ_DECOUPLED_WEIGHT_DECAY", "KVQ_LR_WARMUP_STEPS", "KVQ_LR_DECAY", "KVQ_LR_TOTAL_STEPS",
       "KVQ_LR_MIN_RATIO")
NAMES = ["enc.emb.word", "enc.emb.ln.w", "enc.emb.ln.b", "enc.0.sa.q.w", "enc.0.sa.q.b", "enc.0.ln2.w", "dec.0.ca.k.w", "head.t.w",
         "head.ln.w", "head.bias", "vq.codebook"]


def _config(model):
    sys.path.insert(0, os.path.join(PKG, "models", model))
    try:
        sys.modules.pop("config", None)
        return importlib.import_module("config")
    finally:
        sys.path.pop(0)
        sys.modules.pop("config", None)


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


# ---- resolution ------------------------------------------------------------------------------------------------------------------
def test_first_match_wins_and_the_rest_is_group_0():
    from kvq.engine import NO_DECAY, TrainEngine, resolve_param_groups
    spec = TrainEngine.check_param_groups([{"match": NO_DECAY, "weight_decay": 0.0}, {"match": "vq.codebook", "lr_scale": 10},
                                           {"match": ["enc.*"], "lr_scale": 0.1}])
    table, group_of = resolve_param_groups(spec, NAMES, 0.01)
    assert [g["group"] for g in table] == [0, 1, 2, 3] and table[0] == dict(group=0, match=[], lr_scale=1.0, weight_decay=0.01,
                                                                            names=["dec.0.ca.k.w", "head.t.w"])
    assert group_of == {"enc.emb.word": 3, "enc.emb.ln.w": 1, "enc.emb.ln.b": 1, "enc.0.sa.q.w": 3, "enc.0.sa.q.b": 1, "enc.0.ln2.w": 1,
                        "dec.0.ca.k.w": 0, "head.t.w": 0, "head.ln.w": 1, "head.bias": 1, "vq.codebook": 2}
    assert (table[1]["lr_scale"], table[1]["weight_decay"]) == (1.0, 0.0)            # defaults: scale 1, the engine's decay
    assert (table[2]["lr_scale"], table[2]["weight_decay"]) == (10.0, 0.01)
    assert (table[3]["lr_scale"], table[3]["weight_decay"]) == (0.1, 0.01)
    # enc.* in front takes the encoder's biases too: the order of the list is the priority
    _, first = resolve_param_groups(TrainEngine.check_param_groups([{"match": "enc.*"}, {"match": NO_DECAY}]), NAMES, 0.0)
    assert first["enc.0.sa.q.b"] == 1 and first["head.bias"] == 2


def test_refusals_name_the_offender():
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine, resolve_param_groups
    check = TrainEngine.check_param_groups
    with pytest.raises(KvqError, match=r"enc\.\*\.typo"):
        resolve_param_groups(check([{"match": ["enc.*", "enc.*.typo"]}]), NAMES, 0.0)
    assert len(check([{"match": f"p{i}"} for i in range(15)])) == 15
    with pytest.raises(KvqError, match="16 groups"):
        check([{"match": f"p{i}"} for i in range(16)])
    for bad, what in (({"match": "a", "lr_scale": -1.0}, "lr_scale"), ({"match": "a", "weight_decay": float("nan")}, "weight_decay"),
                      ({"match": "a", "lr_scale": float("inf")}, "lr_scale"), ({"match": "a", "weight_decay": True}, "weight_decay"),
                      ({"match": "a", "lr": 1.0}, "param_groups"), ({"lr_scale": 1.0}, "param_groups"), ({"match": []}, "match"),
                      ({"match": [3]}, "match"), ("enc.*", "param_groups")):
        with pytest.raises(KvqError, match=what):
            check([bad])
    with pytest.raises(KvqError, match="param_groups"):
        check({"match": "a"})
    assert check([{"match": "a", "lr_scale": 0}]) == [dict(match=["a"], lr_scale=0.0, weight_decay=None)]      # 0 is allowed: not frozen
    assert check(None) is None and check([]) == []


# ---- the block table -------------------------------------------------------------------------------------------------------------
def test_block_table_builder_on_a_synthetic_layout():
    from kvq._ffi import KvqError
    from kvq.engine import param_group_blocks, range_group
    # (name, first element): sizes 40 (padded to 48), 16, 7 (padded to 16), 1024, 100 (padded to 112), buffer end padded
    layout = [("a.w", 0), ("a.b", 48), ("a.ln.w", 64), ("b.w", 80), ("b.b", 1104)]
    n = 1216
    group_of = {"a.w": 2, "a.b": 1, "a.ln.w": 1, "b.w": 0, "b.b": 3}
    blocks = param_group_blocks(layout, n, group_of)
    assert blocks.dtype == torch.uint8 and blocks.numel() == n // 16 and not blocks.is_cuda
    ends = [o for _, o in layout[1:]] + [n]
    for (name, o), e in zip(layout, ends):
        assert bool((blocks[o // 16:e // 16] == group_of[name]).all()), name          # the entry's blocks and its padding's
    assert blocks.tolist() == [2] * 3 + [1] + [1] + [0] * 64 + [3] * 7
    assert range_group(blocks, 80, 1104) == 0 and range_group(blocks, 48, 80) == 1 and range_group(blocks, 1104, 1216) == 3
    assert range_group(blocks, 0, 64) is None and range_group(blocks, 64, 96) is None and range_group(blocks, 0, n) is None
    assert range_group(blocks, 96, 112) == 0
    with pytest.raises(KvqError):
        param_group_blocks([("a", 0), ("b", 24)], 48, {"a": 0, "b": 0})
    with pytest.raises(KvqError):
        param_group_blocks([("a", 32), ("b", 16)], 48, {"a": 0, "b": 0})


# ---- options ---------------------------------------------------------------------------------------------------------------------
def test_option_validation_and_environment(monkeypatch):
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine as E
    assert E.check_param_groups(None, env=True) is None and E.check_decoupled_weight_decay(None, env=True) is False
    assert E.check_lr_warmup_steps(None, env=True) == 0 and E.check_lr_decay(None, env=True) is None
    assert E.check_lr_total_steps(None, env=True) is None and E.check_lr_min_ratio(None, env=True) is None
    monkeypatch.setenv("KVQ_PARAM_GROUPS", json.dumps([{"match": ["*.b"], "weight_decay": 0.0}]))
    assert E.check_param_groups(None, env=True) == [dict(match=["*.b"], lr_scale=1.0, weight_decay=0.0)] and E.check_param_groups(None) is None
    for text in ("{not json", json.dumps({"match": "a"}), json.dumps([{"match": "a", "lr_scale": -1}])):
        monkeypatch.setenv("KVQ_PARAM_GROUPS", text)
        with pytest.raises(KvqError, match="param_groups|KVQ_PARAM_GROUPS"):
            E.check_param_groups(None, env=True)
    monkeypatch.setenv("KVQ_PARAM_GROUPS", "")
    assert E.check_param_groups(None, env=True) is None
    for name, check, good, bad_env, bad in (
            ("KVQ_DECOUPLED_WD", E.check_decoupled_weight_decay, ("1", True), ("yes", "2"), (1, "1")),
            ("KVQ_LR_WARMUP_STEPS", E.check_lr_warmup_steps, ("5", 5), ("-1", "x", "1.5"), (-1, 1.5, True)),
            ("KVQ_LR_DECAY", E.check_lr_decay, ("cosine", "cosine"), ("exp",), ("exp", 1)),
            ("KVQ_LR_TOTAL_STEPS", E.check_lr_total_steps, ("9", 9), ("0", "x"), (0, 2.0, True)),
            ("KVQ_LR_MIN_RATIO", E.check_lr_min_ratio, ("0.25", 0.25), ("-0.1", "1.5", "x", "nan"), (-0.1, 1.5, True, "0.1"))):
        monkeypatch.setenv(name, good[0])
        assert check(None, env=True) == good[1]
        monkeypatch.setenv(name, "")
        assert check(None, env=True) == check(None)                              # empty: unset
        for text in bad_env:
            monkeypatch.setenv(name, text)
            with pytest.raises(KvqError):
                check(None, env=True)
        monkeypatch.delenv(name)
        for v in bad:
            with pytest.raises(KvqError):
                check(v)
    assert E.check_lr_decay("none") is None and E.check_lr_decay("linear") == "linear"
    sched = E.check_lr_schedule
    assert sched(0, None, None, None) is None and sched(3, None, None, None) == (3, "none", 0, 0.0)
    assert sched(3, "cosine", 6, None) == (3, "cosine", 6, 0.0) and sched(0, "linear", 6, 0.5) == (0, "linear", 6, 0.5)
    for args in ((3, "cosine", None, None), (3, "cosine", 3, None), (0, None, 6, None), (0, None, None, 0.1)):
        with pytest.raises(KvqError, match="lr_"):
            sched(*args)


def test_the_preset_is_the_bert_recipe():
    from kvq.engine import NO_DECAY, TrainEngine, resolve_param_groups
    _, group_of = resolve_param_groups(TrainEngine.check_param_groups([{"match": NO_DECAY, "weight_decay": 0.0}]), NAMES, 0.01)
    assert {n for n, j in group_of.items() if j == 1} == {"enc.emb.ln.w", "enc.emb.ln.b", "enc.0.sa.q.b", "enc.0.ln2.w", "head.ln.w", "head.bias"}
    json.dumps(NO_DECAY)


# ---- entry points ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["shelgon3", "bagon"])
def test_config_surface(model, monkeypatch):
    cfg = _config(model)
    conf = cfg.get_config()
    assert (cfg.PARAM_GROUPS, cfg.DECOUPLED_WEIGHT_DECAY, cfg.LR_WARMUP_STEPS, cfg.LR_DECAY, cfg.LR_TOTAL_STEPS, cfg.LR_MIN_RATIO) == \
        (None, False, 0, None, None, None)
    assert {k: conf[k] for k in ("param_groups", "decoupled_weight_decay", "lr_warmup_steps", "lr_decay", "lr_total_steps", "lr_min_ratio")} == \
        dict(param_groups=None, decoupled_weight_decay=False, lr_warmup_steps=0, lr_decay=None, lr_total_steps=None, lr_min_ratio=None)
    groups = [{"match": ["*.b", "*.ln.w"], "weight_decay": 0.0}, {"match": "vq.codebook", "lr_scale": 10}]
    monkeypatch.setenv("KVQ_PARAM_GROUPS", json.dumps(groups))
    monkeypatch.setenv("KVQ_DECOUPLED_WD", "1")
    monkeypatch.setenv("KVQ_LR_WARMUP_STEPS", "3")
    monkeypatch.setenv("KVQ_LR_DECAY", "cosine")
    monkeypatch.setenv("KVQ_LR_TOTAL_STEPS", "6")
    monkeypatch.setenv("KVQ_LR_MIN_RATIO", "0.1")
    cfg = _config(model)
    assert cfg.PARAM_GROUPS == groups and cfg.DECOUPLED_WEIGHT_DECAY is True
    assert (cfg.LR_WARMUP_STEPS, cfg.LR_DECAY, cfg.LR_TOTAL_STEPS, cfg.LR_MIN_RATIO) == (3, "cosine", 6, 0.1)
    assert json.loads(json.dumps(cfg.get_config()))["param_groups"] == groups
    for name, bad, what in (("KVQ_PARAM_GROUPS", "[{\"match\": 3}]", "PARAM_GROUPS"), ("KVQ_PARAM_GROUPS", "{oops", "PARAM_GROUPS"),
                            ("KVQ_PARAM_GROUPS", json.dumps([{"match": "a", "lr_scale": -1}]), "PARAM_GROUPS"),
                            ("KVQ_PARAM_GROUPS", json.dumps([{"match": f"p{i}"} for i in range(16)]), "PARAM_GROUPS"),
                            ("KVQ_DECOUPLED_WD", "maybe", "DECOUPLED_WEIGHT_DECAY"), ("KVQ_LR_WARMUP_STEPS", "-1", "LR_WARMUP_STEPS"),
                            ("KVQ_LR_DECAY", "exp", "LR_DECAY"), ("KVQ_LR_TOTAL_STEPS", "3", "LR_TOTAL_STEPS"),
                            ("KVQ_LR_MIN_RATIO", "1.5", "LR_MIN_RATIO")):
        old = os.environ[name]
        monkeypatch.setenv(name, bad)
        with pytest.raises(ValueError, match=what):
            _config(model)
        monkeypatch.setenv(name, old)
    monkeypatch.delenv("KVQ_LR_DECAY")
    with pytest.raises(ValueError, match="LR_TOTAL_STEPS"):                      # a total without a decay means nothing
        _config(model)
    for k in ENV:
        monkeypatch.setenv(k, "")                                                # empty: unset, as TrainEngine reads the variables
    cfg = _config(model)
    assert (cfg.PARAM_GROUPS, cfg.DECOUPLED_WEIGHT_DECAY, cfg.LR_WARMUP_STEPS, cfg.LR_DECAY, cfg.LR_TOTAL_STEPS, cfg.LR_MIN_RATIO) == \
        (None, False, 0, None, None, None)


@pytest.mark.parametrize("model", ["shelgon3", "bagon"])
def test_main_hands_the_options_to_the_engine_and_refuses_them_without_it(model):
    main = open(os.path.join(PKG, "models", model, "main.py")).read()
    for kw in ("param_groups=PARAM_GROUPS", "decoupled_weight_decay=DECOUPLED_WEIGHT_DECAY", "lr_warmup_steps=LR_WARMUP_STEPS",
               "lr_decay=LR_DECAY", "lr_total_steps=LR_TOTAL_STEPS", "lr_min_ratio=LR_MIN_RATIO"):
        assert kw in main, kw
    assert re.search(r"if engine is None and \(PARAM_GROUPS is not None or DECOUPLED_WEIGHT_DECAY or LR_WARMUP_STEPS > 0 or LR_DECAY is not None\):"
                     r"\n(\s+#.*\n)*\s+raise SystemExit\(.*PARAM_GROUPS.*needs? the engine", main)
    trainer = open(os.path.join(PKG, "models", model, "Trainer.py")).read()
    assert "param_groups_line(engine)" in trainer and "lr_epoch_record(engine" in trainer


def test_runlog_lines():
    from kvq.runlog import lr_epoch_record, param_groups_line

    class Eng:
        _pg, decoupled_wd, lr_schedule = {}, True, (3, "cosine", 6, 0.0)

        def param_group_table(self):
            return [dict(group=0, match=[], lr_scale=1.0, weight_decay=0.01, names=2, elements=100),
                    dict(group=1, match=["*.b", "head.bias"], lr_scale=0.1, weight_decay=0.0, names=3, elements=48)]

    line = param_groups_line(Eng())
    assert "decoupled" in line and "*.b, head.bias lr x0.1 wd 0 48 elements" in line and "(everything else) lr x1 wd 0.01 100 elements" in line
    assert param_groups_line(None) is None and lr_epoch_record(None, 1.0) is None
    assert lr_epoch_record(Eng(), torch.tensor(2.5e-4)) == {"train/lr": pytest.approx(2.5e-4)} and lr_epoch_record(Eng(), None) is None
    Eng._pg = Eng.lr_schedule = None
    assert param_groups_line(Eng()) is None and lr_epoch_record(Eng(), 1.0) is None
