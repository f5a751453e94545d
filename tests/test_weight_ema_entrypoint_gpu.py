"""WEIGHT_EMA_DECAY through models/shelgon3/main.py, on the tiny configuration of tests/test_entrypoints_gpu.py (synthetic corpus, one
epoch of 12 steps): validation runs under the average, so the best-val checkpoint holds the AVERAGED weights -- flat.ema and the
aux average of the training state written at the end of that epoch, outside the scope --, the training state holds the live ones,
the epoch's log line reports decay and update count, and the run finishes its test stage."""
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
DECAY = 0.99


def _words(t):
    t = t.detach().cpu().contiguous().reshape(-1)
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def test_best_val_checkpoint_holds_the_average_and_the_run_finishes_its_test_stage(tmp_path):
    base = tmp_path
    data = str(base / "data")
    init = base / "codebook_init.pth"
    g = torch.Generator().manual_seed(11)
    torch.save({"codebook_init_values": (torch.rand(32, 128, generator=g) * 2 - 1) / 32}, str(init))
    env = dict(os.environ)
    env.pop("KVQ_WEIGHT_EMA", None)
    env.update({
        "PYTHONPATH": os.pathsep.join([PKG] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])),
        "KVQ_SYNTHETIC_SENTENCES": "640", "KVQ_BATCH_SIZE": "32", "KVQ_N_EPOCHS": "1", "KVQ_TOKENIZED_SENTENCE_MAX_LENGTH": "12",
        "KVQ_ENCODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_DECODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_LR": "1e-3",
        "KVQ_RUNS_DIR": repr(str(base / "runs")), "KVQ_EXPORT_TRAIN_STATE": "True", "KVQ_MODEL_MODE": "'full'",
        "KVQ_SENTENCES_PATH": repr(data + "/dSentences_sentences_clean.npy"), "KVQ_DATASET_PATH": repr(data + "/dSentences_sentences_clean.npy"),
        "KVQ_LATENT_CLASSES_LABELS_PATH": repr(data + "/dSentences_latent_classes_labels_clean.npy"),
        "KVQ_LATENT_CLASSES_ONE_HOT_PATH": repr(data + "/dSentences_latent_classes_one_hot_clean.npy"),
        "KVQ_VQ_N_E": "32", "KVQ_VQ_E_DIM": "128", "KVQ_VQ_CODEBOOK_INIT_VALUES_PATH": repr(str(init)),
        "KVQ_WEIGHT_EMA_DECAY": str(DECAY)})
    r = subprocess.run([sys.executable, os.path.join(PKG, "models/shelgon3/main.py")], env=env, cwd=str(base), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    runs = glob.glob(str(base / "runs" / "*"))
    assert len(runs) == 1, runs
    run = runs[0]
    assert json.load(open(run + "/run_conf.json"))["weight_ema"] == DECAY
    logs = [json.loads(l) for l in open(run + "/metrics.jsonl")]
    rec = [l for l in logs if "train/weight_ema_updates" in l]
    assert len(rec) == 1 and rec[0]["train/weight_ema_updates"] == STEPS_PER_EPOCH          # one record per epoch
    assert rec[0]["train/weight_ema_decay"] == pytest.approx(12 / 21, rel=1e-6)             # min(0.99, (1 + 11) / (10 + 11))
    assert "weight EMA decay" in r.stdout and f"updates: {STEPS_PER_EPOCH}" in r.stdout
    assert any("val/loss_recon" in l for l in logs) and any("test/loss_recon" in l for l in logs), "the run did not finish its test stage"

    state = torch.load(f"{run}/shelgon_train_state_last.pth", weights_only=True)
    eng, live = state["engine"], state["model_state_dict"]
    assert eng["fingerprint"]["weight_ema"] == DECAY and eng["host"]["step"] == STEPS_PER_EPOCH
    assert eng["structs"]["weight_ema"].tolist()[0] == STEPS_PER_EPOCH
    ckpt = torch.load(f"{run}/shelgon_ckpt_loss_recon_val_best.pth", map_location="cpu")["model_state_dict"]
    assert set(ckpt) == set(live)
    # the flat master buffer IS the parameters' storage: the model_state_dict of the training state (saved outside the scope: the
    # live weights) names each layout entry by its words
    by_words = {}
    for k, v in live.items():
        by_words.setdefault(bytes(_words(v).numpy().tobytes()), []).append(k)
    master, ema = eng["flat"]["master"], eng["flat"]["ema"]
    checked, moved = set(), 0
    for name, o, n, trainable in eng["fingerprint"]["layout"]:
        keys = by_words.get(bytes(_words(master[o:o + n]).numpy().tobytes()))
        assert keys, f"{name}: no parameter of the saved model holds the master buffer's words"
        for k in keys:
            want = ema[o:o + n] if trainable else master[o:o + n]
            assert torch.equal(_words(ckpt[k]), _words(want)), f"{k} ({name}): the best-val checkpoint does not hold the average"
            moved += int(trainable and not torch.equal(_words(ckpt[k]), _words(live[k])))
            checked.add(k)
    for a in eng["aux"]:                                                          # the codebook
        keys = by_words.get(bytes(_words(a["p"]).numpy().tobytes()))
        assert keys
        for k in keys:
            assert torch.equal(_words(ckpt[k]), _words(a["ema"])), f"{k}: the checkpoint's codebook is not its average"
            assert not torch.equal(_words(ckpt[k]), _words(live[k]))
            checked.add(k)
    trained = {k for k, v in live.items() if v.is_floating_point() and "pooler" not in k and "position_ids" not in k}
    assert trained <= checked, sorted(trained - checked)[:8]
    assert moved > 50, "the checkpoint holds the live weights"
