"""RESUME_FROM / EXPORT_TRAIN_STATE of the entry points (models/shelgon3/main.py, models/bagon/main.py), on the tiny configuration of
tests/test_entrypoints_gpu.py: a run of one epoch continued by a second process to three epochs, in the SAME run directory,
against an uninterrupted run of three -- the engine entries of the two training-state files bit for bit, the logged losses as
floats.  The autograd path (USE_ENGINE=False): epochs, optimiser step count and scheduler position continue (no numeric claim:
its products run in vendor libraries).  A RESUME_FROM under another BATCH_SIZE is refused."""
import glob
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")
STEPS_PER_EPOCH = 12          # 640 sentences x 0.6 / 32


def _main(script, base, runs, n_epochs, extra, expect_ok=True):
    env = dict(os.environ)
    data = str(base / "data")
    env.update({
        "PYTHONPATH": os.pathsep.join([PKG] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])),
        "KVQ_SYNTHETIC_SENTENCES": "640", "KVQ_BATCH_SIZE": "32", "KVQ_N_EPOCHS": str(n_epochs), "KVQ_TOKENIZED_SENTENCE_MAX_LENGTH": "12",
        "KVQ_ENCODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_DECODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_LR": "1e-3",
        "KVQ_RUNS_DIR": repr(str(base / runs)), "KVQ_EXPORT_TRAIN_STATE": "True",
        "KVQ_SENTENCES_PATH": repr(data + "/dSentences_sentences_clean.npy"), "KVQ_DATASET_PATH": repr(data + "/dSentences_sentences_clean.npy"),
        "KVQ_LATENT_CLASSES_LABELS_PATH": repr(data + "/dSentences_latent_classes_labels_clean.npy"),
        "KVQ_LATENT_CLASSES_ONE_HOT_PATH": repr(data + "/dSentences_latent_classes_one_hot_clean.npy"),
        "KVQ_VQ_N_E": "32", "KVQ_VQ_E_DIM": "128"})
    if "bagon" in script:
        env["KVQ_MODEL_MODE"] = "'dec-head-ft'"
    else:
        # models/shelgon3/main.py builds its quantiser BEFORE it seeds torch (the codebook's uniform initialisation differs from
        # process to process): runs that are to be compared start from one codebook file, as VQ_CODEBOOK_INIT_VALUES_PATH provides
        init = base / "codebook_init.pth"
        if not init.exists():
            g = torch.Generator().manual_seed(11)
            torch.save({"codebook_init_values": (torch.rand(32, 128, generator=g) * 2 - 1) / 32}, str(init))
        env["KVQ_VQ_CODEBOOK_INIT_VALUES_PATH"] = repr(str(init))
    env.update(extra)
    r = subprocess.run([sys.executable, os.path.join(PKG, script)], env=env, cwd=str(base), capture_output=True, text=True, timeout=600)
    if expect_ok:
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _one_run(base, runs):
    found = glob.glob(str(base / runs / "*"))
    assert len(found) == 1, found                                     # one run directory, resumed or not
    return found[0]


def _metric(run, key):
    """{epoch: value} of a logged key, and the whole log."""
    logs = [json.loads(l) for l in open(run + "/metrics.jsonl")]
    return {l["epoch"]: l[key] for l in logs if key in l}, logs


def _assert_same(a, b, where="engine"):
    assert type(a) is type(b), (where, type(a), type(b))
    if isinstance(a, dict):
        assert set(a) == set(b), (where, sorted(set(a) ^ set(b)))
        for k in a:
            _assert_same(a[k], b[k], f"{where}.{k}")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same(x, y, f"{where}[{i}]")
    elif torch.is_tensor(a):
        raw = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).view(raw), b.reshape(-1).view(raw)), f"{where}: bits differ"
    else:
        assert a == b, (where, a, b)


@pytest.fixture(scope="module")
def shelgon_y(tmp_path_factory):
    """Run Y of the Shelgon case: one epoch with EXPORT_TRAIN_STATE -- continued by the round-trip test, refused by the batch-size one."""
    base = tmp_path_factory.mktemp("shelgon_resume")
    _main("models/shelgon3/main.py", base, "runs_y", 1, {})
    return base, _one_run(base, "runs_y")


def _resume_against_uninterrupted(script, prefix, base, run_y):
    _main(script, base, "runs_x", 3, {})                                             # run X: three epochs, never interrupted
    run_x = _one_run(base, "runs_x")
    y1 = torch.load(f"{run_y}/{prefix}_train_state_last.pth", weights_only=True)
    assert y1["trainer"]["epoch"] == 1 and y1["engine"]["host"]["step"] == STEPS_PER_EPOCH
    conf_before = open(run_y + "/run_conf.json").read()
    _main(script, base, "runs_y", 3, {"KVQ_RESUME_FROM": repr(run_y)})              # a second process continues Y into the same directory
    assert _one_run(base, "runs_y") == run_y and open(run_y + "/run_conf.json").read() == conf_before
    x = torch.load(f"{run_x}/{prefix}_train_state_last.pth", weights_only=True)
    y = torch.load(f"{run_y}/{prefix}_train_state_last.pth", weights_only=True)
    assert set(x) == {"format", "model_state_dict", "engine", "trainer", "rng", "config"}
    _assert_same(x["engine"], y["engine"])
    assert y["engine"]["host"]["step"] == 3 * STEPS_PER_EPOCH
    assert x["trainer"]["epoch"] == y["trainer"]["epoch"] == 3 and x["trainer"]["stats_val_best"] == y["trainer"]["stats_val_best"]
    assert len(y["trainer"]["history"]) == 3 and y["trainer"]["loader_epoch"] == 3
    assert y["config"]["run_id"] == os.path.basename(run_y)
    for key in ("train/loss_recon", "val/loss_recon"):
        mx, _ = _metric(run_x, key)
        my, logs = _metric(run_y, key)
        print(key, mx, my)
        assert sorted(mx) == sorted(my) == [1, 2, 3] and all(mx[e] == my[e] for e in mx), (key, mx, my)
    assert [l["resumed_after_epoch"] for l in logs if "resumed_after_epoch" in l] == [1]
    _assert_same(x["model_state_dict"], y["model_state_dict"], "model_state_dict")
    # the file reads like a best-val checkpoint: the reference's keys
    ckpt = torch.load(glob.glob(f"{run_y}/{prefix}_ckpt_loss_recon_val_best.pth")[0], map_location="cpu")
    assert set(ckpt["model_state_dict"]) == set(y["model_state_dict"])
    return run_y


def test_shelgon_resumed_run_equals_the_uninterrupted_one(shelgon_y):
    base, run_y = shelgon_y
    _resume_against_uninterrupted("models/shelgon3/main.py", "shelgon", base, run_y)
    # N_EPOCHS not larger than the stored epoch: straight to the test stage, no epoch is trained again
    n_before = len(open(run_y + "/metrics.jsonl").readlines())
    _main("models/shelgon3/main.py", base, "runs_y", 3, {"KVQ_RESUME_FROM": repr(run_y + "/shelgon_train_state_last.pth")})
    logs = [json.loads(l) for l in open(run_y + "/metrics.jsonl")][n_before:]
    assert not any("train/loss_recon" in l for l in logs) and any("test/loss_recon" in l for l in logs)
    assert [l["resumed_after_epoch"] for l in logs if "resumed_after_epoch" in l] == [3]


def test_bagon_resumed_run_equals_the_uninterrupted_one(tmp_path):
    _main("models/bagon/main.py", tmp_path, "runs_y", 1, {})
    _resume_against_uninterrupted("models/bagon/main.py", "bagon", tmp_path, _one_run(tmp_path, "runs_y"))


def test_autograd_path_continues_epochs_optimiser_and_scheduler(tmp_path):
    extra = {"KVQ_USE_ENGINE": "False", "KVQ_TOKEN_CACHE": "False"}
    _main("models/shelgon3/main.py", tmp_path, "runs_y", 1, extra)
    run = _one_run(tmp_path, "runs_y")
    first = torch.load(run + "/shelgon_train_state_last.pth", weights_only=True)
    assert "engine" not in first and first["lr_scheduler"]["last_epoch"] == STEPS_PER_EPOCH and first["trainer"]["loader_epoch"] is None
    assert {int(s["step"]) for s in first["optimizer"]["state"].values()} == {STEPS_PER_EPOCH}
    _main("models/shelgon3/main.py", tmp_path, "runs_y", 3, dict(extra, KVQ_RESUME_FROM=repr(run)))
    assert _one_run(tmp_path, "runs_y") == run
    last = torch.load(run + "/shelgon_train_state_last.pth", weights_only=True)
    assert last["trainer"]["epoch"] == 3 and len(last["trainer"]["history"]) == 3
    assert last["lr_scheduler"]["last_epoch"] == 3 * STEPS_PER_EPOCH                     # continued from 12, not restarted at 0
    assert {int(s["step"]) for s in last["optimizer"]["state"].values()} == {3 * STEPS_PER_EPOCH}
    logs = [json.loads(l) for l in open(run + "/metrics.jsonl")]
    at = next(i for i, l in enumerate(logs) if "resumed_after_epoch" in l)
    assert logs[at]["resumed_after_epoch"] == 1
    assert [l["epoch"] for l in logs[:at] if "train/loss_recon" in l] == [1]
    assert [l["epoch"] for l in logs[at:] if "train/loss_recon" in l] == [2, 3]          # the resumed run numbers its epochs 2 - 3
    assert [l["epoch"] for l in logs[at:] if "val/loss_recon" in l] == [2, 3]


def test_resume_under_another_batch_size_is_refused(shelgon_y):
    base, run_y = shelgon_y
    before = {f: os.path.getmtime(os.path.join(run_y, f)) for f in os.listdir(run_y)}
    r = _main("models/shelgon3/main.py", base, "runs_y", 3, {"KVQ_RESUME_FROM": repr(run_y), "KVQ_BATCH_SIZE": "16"}, expect_ok=False)
    assert r.returncode != 0 and "batch_size" in r.stderr and "stored 32, now 16" in r.stderr, r.stderr[-2000:]
    assert {f: os.path.getmtime(os.path.join(run_y, f)) for f in os.listdir(run_y)} == before      # nothing of the stored run was touched
    assert _one_run(base, "runs_y") == run_y
