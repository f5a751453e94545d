"""Cost of the training-state file (kvq/train_state.py) at bert-base widths, beside the duration of an epoch
of the default configuration (models/shelgon3/config.py: 65536 synthetic sentences, 60 / 20 / 20 split, batch 256, 32 tokens,
512 codes): wall time of one save and of one load, and the file's size.  Prints one JSON line; profiles/train_state.md records it.

    PYTHONPATH=kindergarten-vq-vae_amd python3 tools/train_state_cost.py [--out FILE.json] [--dir DIRECTORY_FOR_THE_STATE_FILE]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--sentences", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq", type=int, default=32)
    a = ap.parse_args()
    from dsentences.synthetic import random_token_batch
    from kvq.engine import TrainEngine
    from kvq.train_state import load_train_state, save_train_state, trainer_state
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer

    def build(seed):
        torch.manual_seed(seed)
        vq = VectorQuantizer(512, 768, 0.25)
        vq.materialize_min_encodings = False
        model = Shelgon("bert-base-uncased", vq, "bert-base-uncased", None, compute_dtype=torch.bfloat16).cuda()
        model.set_mode("full")
        return model

    sync = torch.cuda.synchronize
    model = build(0).train()
    eng = TrainEngine(model, lr=1e-4)
    ids, mask = (t.cuda() for t in random_token_batch(a.batch, a.seq, torch.Generator().manual_seed(0)))
    n_train, n_val = int(a.sentences * 0.6) // a.batch + (int(a.sentences * 0.6) % a.batch > 0), \
        int(a.sentences * 0.2) // a.batch + (int(a.sentences * 0.2) % a.batch > 0)
    for _ in range(5):                                            # two eager steps, the capture, two replays
        eng.train_step(ids, mask)
    sync()
    t0 = time.perf_counter()
    for _ in range(n_train):
        eng.train_step(ids, mask)
    sync()
    t_train = time.perf_counter() - t0
    model.eval()
    eng.eval_step(ids, mask)
    sync()
    t0 = time.perf_counter()
    for _ in range(n_val):
        eng.eval_step(ids, mask)
    sync()
    t_val = time.perf_counter() - t0
    model.train()

    t0 = time.perf_counter()
    st = eng.state_dict()
    t_state_dict = time.perf_counter() - t0
    del st
    res = {"params_flat": int(eng.flat.n), "train_steps_per_epoch": n_train, "val_steps_per_epoch": n_val,
           "epoch_train_s": t_train, "epoch_val_s": t_val, "engine_state_dict_s": t_state_dict}
    with tempfile.TemporaryDirectory(dir=a.dir) as tmp:
        path = os.path.join(tmp, "shelgon_train_state_last.pth")
        trainer = trainer_state(1, {}, {}, [], 0, [], None)
        t0 = time.perf_counter()
        save_train_state(path, model, trainer, {"batch_size": a.batch}, engine=eng)
        res["save_s"] = time.perf_counter() - t0
        res["file_bytes"] = os.path.getsize(path)
        del eng, model
        model = build(1).train()
        eng = TrainEngine(model, lr=1e-4)
        sync()
        t0 = time.perf_counter()
        state = load_train_state(path, "cpu")
        res["load_file_s"] = time.perf_counter() - t0
        model.load_state_dict(state["model_state_dict"])
        eng.load_state_dict(state["engine"])
        sync()
        res["load_s"] = time.perf_counter() - t0
    res["step_after_load"] = eng.step_count
    out = eng.train_step(ids, mask)
    res["loss_after_load"] = float(out["loss_recon"])
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
