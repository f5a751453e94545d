"""Host side of the free-running evaluation (FREE_RUNNING_EVAL), no GPU: the option in both configurations,
the refusals of both main.py before any training, the test stage of both trainers with a stub engine (what it hands
TrainEngine.reconstruct, what the stage's record, log dict and decoded rows gain, and that nothing changes with the option off),
and analyses/get_max_acc_sentences.py with FREE_RUNNING."""
import importlib
import importlib.util
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")
SUBS = ("shelgon3", "bagon")
OPTION_VARS = ("KVQ_FREE_RUNNING_EVAL", "KVQ_FREE_RUNNING_EVAL_VAL", "KVQ_FREE_RUNNING_EVAL_BEAMS", "KVQ_DECODER_NEXT_TOKEN", "KVQ_USE_ENGINE",
               "WORLD_SIZE")


class model_dir:
    """`config` / main.py of one model directory importable, under the given environment; everything put back on exit"""

    def __init__(self, sub, **env):
        self.dir, self.env = os.path.join(PKG, "models", sub), env

    def __enter__(self):
        self.path, self.old = list(sys.path), {k: os.environ.get(k) for k in OPTION_VARS}
        for k in OPTION_VARS:
            os.environ.pop(k, None)
        os.environ.update(self.env)
        sys.modules.pop("config", None)
        sys.path.insert(0, self.dir)
        return self

    def main_module(self):
        spec = importlib.util.spec_from_file_location(f"_main_of_{os.path.basename(self.dir)}", os.path.join(self.dir, "main.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    def __exit__(self, *exc):
        sys.path[:] = self.path
        sys.modules.pop("config", None)
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@pytest.mark.parametrize("sub", SUBS)
def test_the_option_is_off_by_default_and_read_from_the_environment(sub):
    with model_dir(sub):
        cfg = importlib.import_module("config")
        assert (cfg.FREE_RUNNING_EVAL, cfg.FREE_RUNNING_EVAL_VAL, cfg.FREE_RUNNING_EVAL_BEAMS) == (False, False, 1)
        conf = cfg.get_config()
        assert (conf["free_running_eval"], conf["free_running_eval_val"], conf["free_running_eval_beams"]) == (False, False, 1)
    with model_dir(sub, KVQ_FREE_RUNNING_EVAL="1", KVQ_FREE_RUNNING_EVAL_VAL="True", KVQ_FREE_RUNNING_EVAL_BEAMS="3"):
        cfg = importlib.import_module("config")
        assert (cfg.FREE_RUNNING_EVAL, cfg.FREE_RUNNING_EVAL_VAL, cfg.FREE_RUNNING_EVAL_BEAMS) == (True, True, 3)
    for env, text in ((dict(KVQ_FREE_RUNNING_EVAL="2"), "FREE_RUNNING_EVAL"), (dict(KVQ_FREE_RUNNING_EVAL_VAL="yes"), "FREE_RUNNING_EVAL_VAL"),
                      (dict(KVQ_FREE_RUNNING_EVAL_BEAMS="9"), "FREE_RUNNING_EVAL_BEAMS"), (dict(KVQ_FREE_RUNNING_EVAL_BEAMS="0"), "FREE_RUNNING_EVAL_BEAMS")):
        with model_dir(sub, **env):
            with pytest.raises(ValueError, match=text):
                importlib.import_module("config")


@pytest.mark.parametrize("sub", SUBS)
def test_main_refuses_the_option_before_any_training(sub):
    for env, text in ((dict(KVQ_FREE_RUNNING_EVAL="True"), "DECODER_NEXT_TOKEN"),
                      (dict(KVQ_FREE_RUNNING_EVAL="True", KVQ_DECODER_NEXT_TOKEN="True", KVQ_USE_ENGINE="False"), "needs the engine"),
                      (dict(KVQ_FREE_RUNNING_EVAL="True", KVQ_DECODER_NEXT_TOKEN="True", WORLD_SIZE="2"), "single process"),
                      (dict(KVQ_FREE_RUNNING_EVAL_VAL="True", KVQ_DECODER_NEXT_TOKEN="True"), "FREE_RUNNING_EVAL_VAL")):
        with model_dir(sub, **env) as d:
            main = d.main_module().main
            with pytest.raises(ValueError, match=text):         # (raised in front of everything else main() does: no device is touched)
                main()


def test_the_refusals_as_a_function():
    from kvq.free_running import check_free_running_config as check
    check(False, False, 1, False, False, 8)                     # off: nothing is asked of the rest
    check(True, True, 4, True, True, 1)
    for args, text in (((True, False, 1, False, True, 1), "DECODER_NEXT_TOKEN"), ((True, False, 1, True, False, 1), "engine"),
                       ((True, False, 1, True, True, 2), "single process"), ((1, False, 1, True, True, 1), "FREE_RUNNING_EVAL"),
                       ((True, False, True, True, True, 1), "BEAMS"), ((True, False, 9, True, True, 1), "BEAMS")):
        with pytest.raises(ValueError, match=text):
            check(*args)


# ---- the test stage of both trainers around a stub engine -----------------------------------------------------------------------
IDS = torch.tensor([[101, 1005, 1006, 102, 0, 0], [101, 1007, 102, 0, 0, 0]])
MASK = (IDS != 0).long()
LABELS = torch.tensor([[0, 1, 0, 2, 1], [1, 2, 1, 0, 0]])


class StubEngine:
    dev = torch.device("cpu")
    weight_ema = None

    def __init__(self):
        self.reconstructs = []

    def eval_step(self, ids, mask, **kw):
        z = torch.zeros(())
        return dict(loss_recon=z, loss_vq=z, perplexity=z, acc=z, acc_per_sentence=torch.zeros(ids.shape[0]), recon_ids=ids)

    def reconstruct(self, enc_ids, enc_mask, start_id, **kw):
        self.reconstructs.append((enc_ids, enc_mask, start_id, kw))
        B = enc_ids.shape[0]
        # sentence 0 comes back whole, sentence 1 with its word replaced: what the kernels would add to the census
        kw["census"].table[0] += torch.tensor([2, 1, 1, 6, 7, 7])
        gen = torch.tensor([[101, 101, 1005, 1006, 102, 0, 0], [101, 101, 1008, 102, 0, 0, 0]])
        rec = dict(dist=torch.tensor([0, 1], dtype=torch.int32), hits=torch.tensor([4, 2], dtype=torch.int32),
                   hyp_len=torch.tensor([4, 3], dtype=torch.int32), ref_len=torch.tensor([4, 3], dtype=torch.int32),
                   exact=torch.tensor([True, False]), n_bad=torch.zeros(1, dtype=torch.int64))
        if kw.get("want_ids"):
            rec.update(ids=gen[:B], lengths=torch.tensor([5, 4]))
        return rec


class Log:
    def __init__(self):
        self.records = []

    def log(self, rec):
        self.records.append(rec)


def _tokenizer():
    from kvq.tokenizer import WordTokenizer
    tok = WordTokenizer(["a", "b", "c", "d"])
    tok.itos.update({1005: "cats", 1006: "sleep", 1007: "dogs", 1008: "birds"})
    return tok


def _stage(sub, free_running, decoded):
    model = SimpleNamespace(decoder_next_token_start_id=101, eval=lambda: None)
    eng = free_running.engine if free_running is not None else StubEngine()
    log, tok = Log(), _tokenizer()
    batches = [dict(input_ids=IDS, attention_mask=MASK, latent_classes_labels=LABELS)] * 2
    if sub == "shelgon3":
        from models.shelgon3.Trainer import test
        run = test(None, None, "cpu", batches, 2, model, tok, True, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, decoded, 2048, 7, log, max_length=6,
                   engine=eng, free_running=free_running)
    else:
        from models.bagon.Trainer import test
        run = test(None, None, "cpu", batches, 2, model, tok, tok, True, 6, True, 6, 0.0, 0.0, decoded, 2048, 2048, 7, log, engine=eng,
                   free_running=free_running)
    return run, log.records[-1], eng


@pytest.mark.parametrize("sub", SUBS)
def test_the_test_stage_reports_the_free_running_numbers(sub):
    from kvq.free_running import FR_KEYS, FreeRunningEval
    off_rows = []
    off_run, off_log, _ = _stage(sub, None, off_rows)
    assert not any(k.startswith("fr_") for k in off_run) and not any("fr_" in k for k in off_log)
    assert not any("free_running_sentence" in r for r in off_rows)

    fr = FreeRunningEval(StubEngine(), 101, eos_id=102, num_beams=1, validation=False, cardinalities=[2, 3, 2, 3, 2])
    assert fr.runs("test") and not fr.runs("val") and not fr.runs("train")
    rows = []
    run, log, eng = _stage(sub, fr, rows)
    assert len(eng.reconstructs) == 2
    enc_ids, enc_mask, start_id, kw = eng.reconstructs[0]
    assert torch.equal(enc_ids, IDS) and torch.equal(enc_mask, MASK) and start_id == 101
    assert kw["eos_id"] == 102 and kw["num_beams"] == 1 and kw["census"] is fr.census and kw["want_ids"] is True
    assert kw["target_ids"] is None and kw["target_mask"] is None          # the autoencoding call: the encoder's ids are the reference
    assert kw["slots"].tolist() == [[0, 1, 4, 6, 10, 12], [0, 2, 5, 7, 8, 11]]
    # two batches of (2 sentences, 1 exact, distance 1, 6 hits, 7 reference tokens)
    assert {k: run[k] for k in FR_KEYS} == {"fr_exact": 0.5, "fr_token_acc": 6 / 7, "fr_edit_rate": 1 / 7}
    assert {k: log[f"test/{k}"] for k in FR_KEYS} == {k: run[k] for k in FR_KEYS}
    assert {k: v for k, v in run.items() if k not in FR_KEYS} == off_run and {k: v for k, v in log.items() if "fr_" not in k} == off_log
    assert len(rows) == 4 and [r["free_running_sentence"] for r in rows[:2]] == ["[CLS] cats sleep [SEP]", "[CLS] birds [SEP]"]
    assert [(r["free_running_edit_distance"], r["free_running_exact"]) for r in rows[:2]] == [(0, True), (1, False)]
    assert [{k: v for k, v in r.items() if not k.startswith("free_running_")} for r in rows] == off_rows


def test_validation_takes_part_only_with_its_own_switch(tmp_path):
    from kvq.free_running import FreeRunningEval, label_cardinalities
    assert label_cardinalities(LABELS) == [2, 3, 2, 3, 2] and label_cardinalities(None) is None
    fr = FreeRunningEval(StubEngine(), 101, validation=True, cardinalities=[2])
    assert fr.runs("val") and fr.runs("test") and not fr.runs("train")
    fr.begin()
    fr.batch(IDS, MASK, labels=LABELS)
    assert fr.engine.reconstructs[0][3]["slots"].tolist() == [[0, 1], [0, 2]] and fr.engine.reconstructs[0][3]["eos_id"] is None
    assert fr.finish() == {"fr_exact": 0.5, "fr_token_acc": 6 / 7, "fr_edit_rate": 1 / 7}
    fr.write_report(str(tmp_path / "reconstruction_by_factor.md"), "test", ["sentence_type"])
    text = (tmp_path / "reconstruction_by_factor.md").read_text().splitlines()
    assert "| all |  | 2 | 0.500000 | 0.857143 | 0.142857 | 1.000000 |" in text
    assert "| sentence_type | 0 | 0 | nan | nan | nan | nan |" in text and "| sentence_type | 1 | 0 | nan | nan | nan | nan |" in text
    fr.begin()
    assert not bool(fr.census.table.any())


# ---- analyses/get_max_acc_sentences.py --------------------------------------------------------------------------------------------
def test_get_max_acc_sentences_filters_on_free_running_exact():
    import pandas as pd
    from analyses.get_max_acc_sentences import max_acc_only
    df = pd.DataFrame({"input_sentence": ["d", "b", "c", "a"], "sentence_acc": [1.0, 1.0, 0.5, 1.0],
                       "free_running_exact": [True, False, True, None]})
    assert max_acc_only(df)["input_sentence"].tolist() == ["a", "b", "d"]
    kept = max_acc_only(df, free_running=True)
    assert kept["input_sentence"].tolist() == ["c", "d"] and kept["index"].tolist() == [2, 0]
    as_text = df.assign(free_running_exact=["True", "False", "true", ""])             # what a .csv round trip leaves
    assert max_acc_only(as_text, free_running=True)["input_sentence"].tolist() == ["c", "d"]
    with pytest.raises(KeyError, match="free_running_exact"):
        max_acc_only(df.drop(columns=["free_running_exact"]), free_running=True)


def test_get_max_acc_sentences_main_reads_the_switch(tmp_path, monkeypatch):
    import pandas as pd
    import analyses.get_max_acc_sentences as G
    pd.DataFrame({"input_sentence": ["b", "a"], "sentence_acc": [1.0, 0.0], "free_running_exact": [False, True]}).to_csv(
        tmp_path / "decoded_sentences.csv", index=False)
    monkeypatch.setattr(G, "RUN_DIR", str(tmp_path))
    monkeypatch.setattr(G, "FREE_RUNNING", False)
    assert G.main()["input_sentence"].tolist() == ["b"]
    monkeypatch.setattr(G, "FREE_RUNNING", True)
    assert G.main()["input_sentence"].tolist() == ["a"]
    pd.DataFrame({"input_sentence": ["b", "a"], "sentence_acc": [1.0, 0.0]}).to_csv(tmp_path / "decoded_sentences.csv", index=False)
    with pytest.raises(KeyError, match="free_running_exact"):
        G.main()
