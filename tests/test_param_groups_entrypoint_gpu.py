"""PARAM_GROUPS, DECOUPLED_WEIGHT_DECAY and a warm-up / cosine schedule through models/shelgon3/main.py and models/bagon/main.py, on
the tiny configuration of tests/test_entrypoints_gpu.py (synthetic corpus, two epochs of 12 steps): the run finishes, run_conf.json
holds the constants, the group table is printed once and every epoch reports its last learning rate."""
import glob
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")
STEPS_PER_EPOCH = 12          # 640 sentences x 0.6 / 32
LR, W, T, RATIO = 1e-3, 4, 24, 0.1
NO_DECAY = {"match": ["*.b", "*.ln.w", "*.ln2.w", "head.bias"], "weight_decay": 0.0}
OPTION_ENV = ("KVQ_PARAM_GROUPS", "KVQ_DECOUPLED_WD", "KVQ_DECOUPLED_WEIGHT_DECAY", "KVQ_LR_WARMUP_STEPS", "KVQ_LR_DECAY", "KVQ_LR_TOTAL_STEPS",
              "KVQ_LR_MIN_RATIO")


def _lr(t):
    x = min(max((t - W) / (T - W), 0.0), 1.0)
    return float(np.float32(LR)) * (t / W if t < W else 1.0) * (RATIO + (1.0 - RATIO) * 0.5 * (1.0 + math.cos(math.pi * x)))


def _run(script, tmp_path, groups, extra):
    env = {k: v for k, v in os.environ.items() if k not in OPTION_ENV}
    data = str(tmp_path / "data")
    env.update({
        "PYTHONPATH": os.pathsep.join([PKG] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])),
        "KVQ_SYNTHETIC_SENTENCES": "640", "KVQ_BATCH_SIZE": "32", "KVQ_N_EPOCHS": "2", "KVQ_TOKENIZED_SENTENCE_MAX_LENGTH": "12",
        "KVQ_ENCODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_DECODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_LR": str(LR), "KVQ_WEIGHT_DECAY": "0.01",
        "KVQ_RUNS_DIR": repr(str(tmp_path / "runs")),
        "KVQ_LATENT_CLASSES_LABELS_PATH": repr(data + "/dSentences_latent_classes_labels_clean.npy"),
        "KVQ_LATENT_CLASSES_ONE_HOT_PATH": repr(data + "/dSentences_latent_classes_one_hot_clean.npy"),
        "KVQ_PARAM_GROUPS": json.dumps(groups), "KVQ_DECOUPLED_WD": "1", "KVQ_LR_WARMUP_STEPS": str(W), "KVQ_LR_DECAY": "cosine",
        "KVQ_LR_TOTAL_STEPS": str(T), "KVQ_LR_MIN_RATIO": str(RATIO)})
    env.update(extra(data))
    r = subprocess.run([sys.executable, os.path.join(PKG, script)], env=env, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    runs = glob.glob(str(tmp_path / "runs" / "*"))
    assert len(runs) == 1
    return runs[0], r.stdout


def _check(run, stdout, groups):
    conf = json.load(open(run + "/run_conf.json"))
    assert conf["param_groups"] == groups and conf["decoupled_weight_decay"] is True and conf["use_engine"]
    assert (conf["lr_warmup_steps"], conf["lr_decay"], conf["lr_total_steps"], conf["lr_min_ratio"]) == (W, "cosine", T, RATIO)
    flat = " ".join(stdout.split())                        # the console wraps long lines
    assert flat.count("parameter groups (decoupled weight decay)") == 1, "the group table is printed once per run"
    assert "(everything else) lr x1 wd 0.01" in flat and "*.b, *.ln.w, *.ln2.w, head.bias lr x1 wd 0 " in flat
    logs = [json.loads(l) for l in open(run + "/metrics.jsonl")]
    lrs = [l["train/lr"] for l in logs if "train/lr" in l]
    assert len(lrs) == 2                                   # one record per epoch: the rate of its last optimiser step
    for got, t in zip(lrs, (STEPS_PER_EPOCH, 2 * STEPS_PER_EPOCH)):
        assert abs(got - _lr(t)) <= 2.0 ** -23 * _lr(t), (t, got, _lr(t))
    assert stdout.count("| lr: ") == 2
    tr = [l["train/loss_recon"] for l in logs if "train/loss_recon" in l]
    assert len(tr) == 2 and all(math.isfinite(v) for v in tr) and tr[1] < tr[0]
    assert any("test/loss_recon" in l for l in logs), "the run did not finish its test stage"
    return flat


def test_shelgon_main_with_groups_decoupled_decay_and_a_schedule(tmp_path):
    groups = [NO_DECAY, {"match": "vq.codebook", "lr_scale": 10}, {"match": "enc.*", "lr_scale": 0.1}]
    run, stdout = _run("models/shelgon3/main.py", tmp_path, groups, lambda d: {
        "KVQ_SENTENCES_PATH": repr(d + "/dSentences_sentences_clean.npy"), "KVQ_VQ_N_E": "32", "KVQ_VQ_E_DIM": "128"})
    flat = _check(run, stdout, groups)
    assert f"vq.codebook lr x10 wd 0.01 {32 * 128} elements" in flat and "enc.* lr x0.1 wd 0.01" in flat


def test_bagon_main_with_groups_decoupled_decay_and_a_schedule(tmp_path):
    groups = [NO_DECAY, {"match": ["dec.*", "head.*"], "lr_scale": 0.5}]
    run, stdout = _run("models/bagon/main.py", tmp_path, groups, lambda d: {
        "KVQ_DATASET_PATH": repr(d + "/dSentences_sentences_clean.npy"), "KVQ_MODEL_MODE": "'dec-head-ft'"})
    flat = _check(run, stdout, groups)
    assert "dec.*, head.* lr x0.5 wd 0.01" in flat
