"""Cost of the grouped Adam entry (kvq_adam_step_grouped) against kvq_adam_step_dev at the benchmarked flat
length (bench.py's default: bert-base-uncased, bf16 gradient, bf16 shadow, mode full), on the buffers of ONE engine in ONE process.
Four arms, alternated window by window after a warm-up, each window timed with device events and at least --window-s long:

  a   kvq_adam_step_dev                                           (today's launch)
  b   kvq_adam_step_grouped, block_group = NULL                   (one group: the same kernel work)
  c   kvq_adam_step_grouped with the engine's block table under   (one byte per 16 elements on top of 28 bytes per element)
      [{"match": NO_DECAY, "weight_decay": 0}]: the group changes at every bias / LayerNorm boundary
  d   arm b with decoupled = 1: the one instantiation family that runs at occupancy 5 instead of 6 (beside one more multiplication)

Arm a runs twice per round (a, b, a2, c, d): |a - a2| over the rounds is the spread a difference has to exceed to mean anything.
Prints one JSON line; profiles/adam_groups.md records it.

    PYTHONPATH=kindergarten-vq-vae_amd python3 tools/adam_groups_cost.py [--out FILE.json] [--rounds 5] [--window-s 1.0]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default="bert-base-uncased")
    ap.add_argument("--codes", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_groups_cost.py needs an MI355X (a time from anything else says nothing)")
    from kvq import nnops
    from kvq.engine import NO_DECAY, TrainEngine
    from models.bagon.Bagon import LOCAL_BERT_CONFIGS
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer

    torch.manual_seed(0)
    hidden = LOCAL_BERT_CONFIGS[a.model].get("hidden_size", 768)
    vq = VectorQuantizer(a.codes, hidden, 0.25)
    vq.materialize_min_encodings = False
    model = Shelgon(a.model, vq, a.model, None, compute_dtype=torch.bfloat16).cuda()
    model.set_mode("full")
    eng = TrainEngine(model.train(), lr=1e-4, weight_decay=0.01, param_groups=[{"match": NO_DECAY, "weight_decay": 0.0}])
    fl, pg = eng.flat, eng._pg
    lo, hi = max(fl.ranges, key=lambda r: r[1] - r[0])            # (mode full: the one range that covers the buffer)
    n = hi - lo
    fl.grad.normal_(0.0, 1e-3)                                     # a gradient that is not all zeros; lr = 1e-4 keeps the weights finite
    nnops.step_state_advance(eng._state, eng.lr, eng.gamma, [], *eng.betas)
    b1, b2 = eng.betas
    views = (fl.master[lo:hi], fl.grad[lo:hi], fl.m[lo:hi], fl.v[lo:hi], eng._state, b1, b2, eng.eps, eng.wd)
    arms = {
        "a": lambda: nnops.adam_step_dev(*views, shadow=fl.shadow[lo:hi]),
        "b": lambda: nnops.adam_step_grouped(*views, shadow=fl.shadow[lo:hi], group_lr_scale=pg["scale"][:1], group_wd=pg["wd"][:1], n_groups=1),
        "c": lambda: nnops.adam_step_grouped(*views, shadow=fl.shadow[lo:hi], block_group=pg["blocks"], first_element=lo,
                                             group_lr_scale=pg["scale"], group_wd=pg["wd"], n_groups=len(pg["table"])),
    }
    arms["d"] = lambda: nnops.adam_step_grouped(*views, shadow=fl.shadow[lo:hi], group_lr_scale=pg["scale"][:1], group_wd=pg["wd"][:1],
                                                n_groups=1, decoupled=True)
    arms["a2"] = arms["a"]
    sync = torch.cuda.synchronize

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) / reps

    for fn in arms.values():                                       # warm-up, and the launch count that fills a window
        window(fn, 20)
    reps = max(20, int(a.window_s * 1e3 / window(arms["a"], 50)) + 1)
    ms = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k in ("a", "b", "a2", "c", "d"):
            ms[k].append(window(arms[k], reps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    blocks = pg["blocks_host"][lo // 16:hi // 16]
    res = {"model": a.model, "elements": int(n), "flat_n": int(fl.n), "launches_per_window": reps, "rounds": a.rounds,
           "group_changes": int((blocks[1:] != blocks[:-1]).sum()), "groups": len(pg["table"]),
           "ms": ms, "ms_median": med,
           "a_vs_a2_spread_pct": max(abs(x - y) / x * 100 for x, y in zip(ms["a"], ms["a2"])),
           "b_vs_a_pct": (med["b"] / med["a"] - 1) * 100, "c_vs_a_pct": (med["c"] / med["a"] - 1) * 100,
           "d_vs_a_pct": (med["d"] / med["a"] - 1) * 100,
           "bytes_a": 28 * n, "bytes_table": int(n // 16), "tb_per_s_a": 28 * n / (med["a"] * 1e-3) / 1e12,
           "finite": bool(torch.isfinite(fl.master[lo:hi]).all()), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
