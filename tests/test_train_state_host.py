"""Host-side checks of resumable training (kvq/train_state.py): the training-state file's keys, its
weights_only load and its atomic write; a TokenCacheLoader whose epoch counter was restored; the three configuration constants;
the readability helper of kvq.ddp on two gloo ranks; the configuration comparison of a resumed run; the trainers' keyword
arguments.  No device needed."""
import importlib
import inspect
import os
import socket
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")


class _StandInEngine:
    """What save_train_state asks of an engine: state_dict() of plain data."""

    def __init__(self, step):
        self.step = step

    def state_dict(self):
        return {"format": 1, "flat": {"master": torch.arange(8, dtype=torch.float32) + self.step},
                "structs": {"state": torch.tensor([self.step, 0, 0])}, "host": {"step": self.step, "grads_are_mean": False},
                "fingerprint": {"layout": [["w", 0, 8, True]], "betas": [0.9, 0.999], "max_grad_norm": float("inf"), "fp8": False}}


def _trainer(epoch):
    import numpy as np
    from kvq.train_state import trainer_state
    best = {"loss_recon_best": np.inf if epoch == 0 else 1.5, "loss_recon_is_best": np.float64(1.0) < np.float64(2.0),
            "metric_acc_best": 0}
    hist = [({"loss_recon_run": 2.0 / e}, {"loss_recon_run": 3.0 / e}) for e in range(1, epoch + 1)]

    class _Loader:
        pass
    dl = _Loader()
    dl.epoch = epoch
    return trainer_state(epoch, best, dict(best), hist, 2, [{"epoch": 1, "stage": "train", "input_sentence": "a b", "recon_sentence": "a c"}], dl)


def test_file_keys_plain_data_and_atomic_write(tmp_path, monkeypatch):
    from kvq import train_state as ts
    model = torch.nn.Linear(4, 3)
    path = str(tmp_path / "x_train_state_last.pth")
    ts.save_train_state(path, model, _trainer(2), {"batch_size": 32, "milestones": (10, 20), "lr": 1e-3}, engine=_StandInEngine(7))
    raw = torch.load(path, weights_only=True)                   # plain data: no pickled objects anywhere in the file
    assert set(raw) == {"format", "model_state_dict", "engine", "trainer", "rng", "config"} and raw["format"] == ts.TRAIN_STATE_FORMAT
    st = ts.load_train_state(path, "cpu")
    assert set(st["model_state_dict"]) == {"weight", "bias"} and torch.equal(st["model_state_dict"]["weight"], model.weight.data)
    assert torch.equal(st["engine"]["flat"]["master"], torch.arange(8, dtype=torch.float32) + 7)
    assert st["engine"]["fingerprint"]["max_grad_norm"] == float("inf") and st["engine"]["host"] == {"step": 7, "grads_are_mean": False}
    tr = st["trainer"]
    assert set(tr) == {"epoch", "stats_train_best", "stats_val_best", "history", "skipped", "decoded_sentences", "loader_epoch"}
    assert tr["epoch"] == 2 and tr["skipped"] == 2 and tr["loader_epoch"] == 2 and tr["stats_val_best"]["loss_recon_best"] == 1.5
    assert tr["stats_val_best"]["loss_recon_is_best"] is True             # a numpy bool became a Python one
    assert tr["history"] == [[{"loss_recon_run": 2.0}, {"loss_recon_run": 3.0}], [{"loss_recon_run": 1.0}, {"loss_recon_run": 1.5}]]
    assert tr["decoded_sentences"][0]["recon_sentence"] == "a c"
    assert st["config"] == {"batch_size": 32, "milestones": [10, 20], "lr": 1e-3}
    assert st["rng"]["cpu"].dtype == torch.uint8 and torch.equal(st["rng"]["cpu"], torch.get_rng_state())
    # the autograd path: optimiser and scheduler instead of the engine
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2, 4], gamma=0.5)
    for _ in range(3):
        opt.zero_grad()
        model(torch.ones(2, 4)).sum().backward()
        opt.step()
        sched.step()
    p2 = str(tmp_path / "autograd.pth")
    ts.save_train_state(p2, model, _trainer(1), {}, opt=opt, lr_sched=sched)
    st2 = ts.load_train_state(p2)
    assert "engine" not in st2 and st2["lr_scheduler"]["last_epoch"] == 3
    opt_b = torch.optim.Adam(model.parameters(), lr=1e-3)
    sched_b = torch.optim.lr_scheduler.MultiStepLR(opt_b, milestones=[2, 4], gamma=0.5)
    ts.load_optimizer(st2, opt_b, sched_b)
    assert sched_b.last_epoch == 3 and opt_b.param_groups[0]["lr"] == opt.param_groups[0]["lr"] == 5e-4
    assert all(int(s["step"]) == 3 for s in opt_b.state.values()) and len(opt_b.state) == 2
    sched_b.step(); sched.step()
    assert opt_b.param_groups[0]["lr"] == opt.param_groups[0]["lr"] == 2.5e-4      # the second milestone still fires
    # atomic: a write that fails leaves the previous file byte for byte, and no temporary behind
    before = open(path, "rb").read()

    def boom(obj, f, *a, **k):
        with open(f, "wb") as fp:
            fp.write(b"half a file")
        raise OSError("disk full")
    monkeypatch.setattr(ts.torch, "save", boom)
    with pytest.raises(OSError, match="disk full"):
        ts.save_train_state(path, model, _trainer(3), {}, engine=_StandInEngine(9))
    monkeypatch.undo()
    assert open(path, "rb").read() == before and not any(f.endswith(".tmp") for f in os.listdir(tmp_path))
    # not a state file / another format
    torch.save({"model_state_dict": {}}, str(tmp_path / "ckpt.pth"))
    with pytest.raises(ts.TrainStateError, match="format"):
        ts.load_train_state(str(tmp_path / "ckpt.pth"))
    with pytest.raises(ts.TrainStateError, match="plain data"):
        ts.save_train_state(str(tmp_path / "bad.pth"), model, {"epoch": {1, 2}}, {}, engine=_StandInEngine(1))
    assert not os.path.exists(tmp_path / "bad.pth")
    assert ts.resolve_path(str(tmp_path), "x_train_state_last.pth") == path and ts.resolve_path(path, "other.pth") == path


def test_restored_trainer_state_and_generators():
    from kvq import train_state as ts
    torch.manual_seed(5)
    torch.rand(3)
    resume = {"trainer": ts._plain(_trainer(2)), "rng": ts.rng_state()}
    want = torch.rand(4)
    torch.manual_seed(99)

    class _Loader:
        epoch = 0
    dl, decoded = _Loader(), [{"stale": True}]
    first, tb, vb, hist, skipped = ts.restore_trainer(resume, decoded, dl)
    assert first == 3 and skipped == 2 and dl.epoch == 2 and tb["loss_recon_best"] == 1.5 and vb == tb
    assert hist == [({"loss_recon_run": 2.0}, {"loss_recon_run": 3.0}), ({"loss_recon_run": 1.0}, {"loss_recon_run": 1.5})]
    assert decoded == [{"epoch": 1, "stage": "train", "input_sentence": "a b", "recon_sentence": "a c"}]       # refilled in place
    assert torch.equal(torch.rand(4), want)                      # the generator continues where the stored run's stood


def test_token_cache_loader_with_a_restored_epoch_yields_the_uninterrupted_permutation():
    from dsentences.token_cache import TokenCache
    ids = torch.arange(1, 1 + 37 * 5).reshape(37, 5)
    cache = TokenCache.from_ids(ids)
    full = cache.loader(8, True, seed=69)
    epochs = [[b["input_ids"].clone() for b in full] for _ in range(3)]
    assert not torch.equal(epochs[0][0], epochs[1][0]) and full.epoch == 3
    resumed = cache.loader(8, True, seed=69)
    resumed.epoch = 2                                            # what restore_trainer sets from the file
    third = [b["input_ids"] for b in resumed]
    assert len(third) == len(epochs[2]) == 5 and all(torch.equal(a, b) for a, b in zip(third, epochs[2]))
    for rank in (0, 1):                                          # and every rank's slice of it
        a, b = cache.loader(4, True, seed=3, rank=rank, world=2), cache.loader(4, True, seed=3, rank=rank, world=2)
        list(a)
        second = [x["input_ids"].clone() for x in a]
        b.epoch = 1
        assert all(torch.equal(x, y["input_ids"]) for x, y in zip(second, b))


def _config(model):
    sys.path.insert(0, os.path.join(PKG, "models", model))
    try:
        sys.modules.pop("config", None)
        return importlib.import_module("config")
    finally:
        sys.path.pop(0)
        sys.modules.pop("config", None)


@pytest.mark.parametrize("model", ["shelgon3", "bagon"])
def test_config_constants_are_validated_like_their_neighbours(model, monkeypatch):
    for k in ("KVQ_EXPORT_TRAIN_STATE", "KVQ_TRAIN_STATE_EVERY_EPOCHS", "KVQ_RESUME_FROM"):
        monkeypatch.delenv(k, raising=False)
    cfg = _config(model)
    assert cfg.EXPORT_TRAIN_STATE is False and cfg.TRAIN_STATE_EVERY_EPOCHS == 1 and cfg.RESUME_FROM is None
    assert {"export_train_state", "train_state_every_epochs", "resume_from"} <= set(cfg.get_config())
    for text, want in (("1", 1), ("5", 5), (" 3 ", 3)):
        monkeypatch.setenv("KVQ_TRAIN_STATE_EVERY_EPOCHS", text)
        cfg = _config(model)
        assert cfg.TRAIN_STATE_EVERY_EPOCHS == want and type(cfg.TRAIN_STATE_EVERY_EPOCHS) is int
    for bad in ("0", "-2", "2.5", "x", "True", "None"):
        monkeypatch.setenv("KVQ_TRAIN_STATE_EVERY_EPOCHS", bad)
        with pytest.raises(ValueError, match="TRAIN_STATE_EVERY_EPOCHS"):
            _config(model)
    monkeypatch.delenv("KVQ_TRAIN_STATE_EVERY_EPOCHS")
    for text, want in (("'/runs/a b'", "/runs/a b"), ("/runs/2026_01_01", "/runs/2026_01_01"), ("", None), ("None", None)):
        monkeypatch.setenv("KVQ_RESUME_FROM", text)
        assert _config(model).RESUME_FROM == want, text
    monkeypatch.setenv("KVQ_RESUME_FROM", "3")
    with pytest.raises(ValueError, match="RESUME_FROM"):
        _config(model)
    monkeypatch.delenv("KVQ_RESUME_FROM")
    monkeypatch.setenv("KVQ_EXPORT_TRAIN_STATE", "True")
    assert _config(model).EXPORT_TRAIN_STATE is True
    monkeypatch.setenv("KVQ_EXPORT_TRAIN_STATE", "yes")
    with pytest.raises(ValueError, match="EXPORT_TRAIN_STATE"):
        _config(model)
    monkeypatch.delenv("KVQ_EXPORT_TRAIN_STATE")
    src = open(os.path.join(PKG, "models", model, "config.py")).read()
    prefix = "shelgon" if model == "shelgon3" else "bagon"
    assert f"{prefix}_train_state_last.pth" in next(l for l in src.splitlines() if l.startswith("EXPORT_TRAIN_STATE = False"))
    main = open(os.path.join(PKG, "models", model, "main.py")).read()
    assert f'"{prefix}_train_state_last.pth"' in main and "readable_everywhere" in main and "resumed_after_epoch" in main


@pytest.mark.parametrize("model", ["shelgon3", "bagon"])
def test_train_takes_the_new_keywords_and_defaults_to_todays_behaviour(model):
    trainer = importlib.import_module(f"models.{model}.Trainer")
    sig = inspect.signature(trainer.train)
    assert sig.parameters["train_state_path"].default is None and sig.parameters["train_state_every"].default == 1 \
        and sig.parameters["resume"].default is None
    from kvq.train_state import check_every
    for bad in (0, -1, 1.5, True, "2", None):
        with pytest.raises(ValueError, match="train_state_every"):
            check_every(bad, "train_state_every")


def test_config_comparison_lists_exactly_the_differing_keys():
    from kvq.train_state import RESUME_CONFIG_KEYS, config_differences
    stored = {"batch_size": 32, "train_split_pct": 0.6, "val_split_pct": 0.2, "ds_gen_seed": 69, "token_cache": True,
              "tokenized_sentence_max_length": 12, "world_size": 1, "n_epochs": 1, "runs_dir": "./a", "lr": 1e-3, "export_checkpoint": True}
    assert set(RESUME_CONFIG_KEYS) == {"batch_size", "train_split_pct", "val_split_pct", "ds_gen_seed", "token_cache",
                                       "tokenized_sentence_max_length", "world_size"}
    assert config_differences(stored, dict(stored)) == []
    # what may differ: extending a run is the point; everything numeric is the engine fingerprint's business
    assert config_differences(stored, dict(stored, n_epochs=3, runs_dir="./b", lr=1e-4, export_checkpoint=False, resume_from="./a/x")) == []
    now = dict(stored, batch_size=16, world_size=2, n_epochs=9)
    diff = config_differences(stored, now)
    assert [d.split(":")[0] for d in diff] == ["batch_size", "world_size"] and "stored 32, now 16" in diff[0]
    for key in RESUME_CONFIG_KEYS:
        changed = dict(stored)
        changed[key] = "other"
        assert [d.split(":")[0] for d in config_differences(stored, changed)] == [key]
    del now["token_cache"]
    assert [d.split(":")[0] for d in config_differences(stored, now)] == ["batch_size", "token_cache", "world_size"]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _readable_worker(rank, world, port, tmp):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    sys.path.insert(0, PKG)
    import torch.distributed as dist
    from kvq import ddp
    dist.init_process_group("gloo", rank=rank, world_size=world)
    shared = os.path.join(tmp, "shared.pth")
    only1 = os.path.join(tmp, "rank1_only.pth")                # "readable here" differs: rank 0 is handed a path that is not there
    got = {"shared": ddp.readable_everywhere(shared),
           "one_rank": ddp.readable_everywhere(only1 if rank == 1 else only1 + ".missing"),
           "nowhere": ddp.readable_everywhere(os.path.join(tmp, "missing.pth")),
           "directory": ddp.readable_everywhere(tmp)}
    torch.save(got, os.path.join(tmp, f"got{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_readability_helper_answers_the_same_on_two_gloo_ranks(tmp_path):
    import torch.multiprocessing as mp
    from kvq import ddp
    for name in ("shared.pth", "rank1_only.pth"):
        (tmp_path / name).write_bytes(b"x")
    assert ddp.readable_everywhere(str(tmp_path / "shared.pth")) is True           # no process group: this process alone
    assert ddp.readable_everywhere(str(tmp_path / "missing.pth")) is False
    mp.spawn(_readable_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = torch.load(tmp_path / "got0.pt"), torch.load(tmp_path / "got1.pt")
    assert a == b == {"shared": True, "one_rank": False, "nowhere": False, "directory": False}
