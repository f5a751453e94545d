"""LOSS_IGNORE_PAD through models/shelgon3/main.py, on the tiny configuration of tests/test_entrypoints_gpu.py (synthetic corpus),
limited to ONE train batch in a fresh child process: the run finishes its test stage, run_conf.json records the switch the step
really ran with, and the logged train accuracy is the real-token accuracy of that batch, recomputed here from the sentences the
run decoded (the word tokenizer writes one word per position, "[PAD]" at pads)."""
import glob
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")
BATCH, S = 32, 12


@pytest.mark.parametrize("use_engine", [True, False])
def test_the_run_logs_the_real_token_accuracy(tmp_path, use_engine):
    """use_engine=False: the autograd path, where Trainer.step hands the pad id to fused_cross_entropy(ignore_index=...)."""
    base = tmp_path
    data = str(base / "data")
    env = dict(os.environ)
    env.update({
        "PYTHONPATH": os.pathsep.join([PKG] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])),
        "KVQ_SYNTHETIC_SENTENCES": "640", "KVQ_BATCH_SIZE": str(BATCH), "KVQ_N_EPOCHS": "1", "KVQ_TOKENIZED_SENTENCE_MAX_LENGTH": str(S),
        "KVQ_ENCODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_DECODER_MODEL_NAME": "'kvq-bert-tiny'", "KVQ_LR": "1e-3",
        "KVQ_RUNS_DIR": repr(str(base / "runs")), "KVQ_MODEL_MODE": "'full'",
        "KVQ_SENTENCES_PATH": repr(data + "/dSentences_sentences_clean.npy"), "KVQ_DATASET_PATH": repr(data + "/dSentences_sentences_clean.npy"),
        "KVQ_LATENT_CLASSES_LABELS_PATH": repr(data + "/dSentences_latent_classes_labels_clean.npy"),
        "KVQ_LATENT_CLASSES_ONE_HOT_PATH": repr(data + "/dSentences_latent_classes_one_hot_clean.npy"),
        "KVQ_VQ_N_E": "32", "KVQ_VQ_E_DIM": "128",
        "KVQ_LIM_BATCHES_TRAIN_PCT": "0.1",           # int(12 * 0.1) = 1 train batch: the epoch's mean IS that batch's value
        "KVQ_USE_ENGINE": str(use_engine), "KVQ_TOKEN_CACHE": str(use_engine),
        "KVQ_LOSS_IGNORE_PAD": "1"})
    r = subprocess.run([sys.executable, os.path.join(PKG, "models/shelgon3/main.py")], env=env, cwd=str(base), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    runs = glob.glob(str(base / "runs" / "*"))
    assert len(runs) == 1, runs
    run = runs[0]
    conf = json.load(open(run + "/run_conf.json"))
    assert conf["loss_ignore_pad"] is True
    logs = [json.loads(l) for l in open(run + "/metrics.jsonl")]
    assert any("val/loss_recon" in l for l in logs) and any("test/loss_recon" in l for l in logs), "the run did not finish its test stage"
    steps = [l["perf/train_steps"] for l in logs if "perf/train_steps" in l]
    assert steps == [1], steps
    logged = [l["train/acc"] for l in logs if "train/acc" in l]
    assert len(logged) == 1

    import pandas as pd
    feather = run + "/decoded_sentences.feather"
    df = pd.read_feather(feather) if os.path.exists(feather) else pd.read_csv(run + "/decoded_sentences.csv")
    rows = df[(df["stage"] == "train") & (df["epoch"] == 1)]
    assert len(rows) == BATCH
    hits = real = same = 0
    for inp, rec in zip(rows["input_sentence"], rows["recon_sentence"]):
        a, b = inp.split(" "), rec.split(" ")
        assert len(a) == len(b) == S
        n_real = sum(w != "[PAD]" for w in a)
        assert 0 < n_real < S, "a sentence without pads or without words"
        for x, y in zip(a, b):
            same += x == y
            if x == "[PAD]":
                assert y == "[PAD]", "recon_ids does not carry the pad id at an ignored place"
            else:
                real += 1
                hits += x == y
    want = 100.0 * hits / real
    assert logged[0] == pytest.approx(want, rel=1e-5, abs=1e-5), (logged[0], want)
    over_all_positions = 100.0 * same / (BATCH * S)
    assert abs(over_all_positions - want) > 10, "this batch cannot tell the two accuracies apart"
