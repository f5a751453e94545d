"""Cost of TrainEngine(weight_ema=...) at the benchmarked shape (bench.py's default: bert-base-uncased, bf16,
256 sentences of 32 tokens, 512 codes, mode full): the time of a replayed training step with the option off and on, measured in
ONE process in alternating blocks, the achieved bandwidth of the update kernel over the flat buffer (12 bytes per element: p and
ema read, ema written), and the Adam kernel's in the same run as the yardstick (28 bytes per element with a bf16 gradient and
shadow: p, m, v read and written, 2 + 2 bytes of gradient and shadow).  Prints one JSON line; profiles/weight_ema.md records it.

    PYTHONPATH=kindergarten-vq-vae_amd python3 tools/weight_ema_cost.py [--out FILE.json] [--steps 40] [--blocks 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default="bert-base-uncased")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq", type=int, default=32)
    ap.add_argument("--codes", type=int, default=512)
    ap.add_argument("--steps", type=int, default=40, help="replayed steps per timed block")
    ap.add_argument("--blocks", type=int, default=3, help="timed blocks per arm, alternating off / on")
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--decay", type=float, default=0.9999)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weight_ema_cost.py needs an MI355X (a time from anything else says nothing)")
    from dsentences.synthetic import random_token_batch
    from kvq import nnops
    from kvq.engine import TrainEngine
    from models.bagon.Bagon import LOCAL_BERT_CONFIGS
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer

    hidden = LOCAL_BERT_CONFIGS[a.model].get("hidden_size", 768)

    def build(weight_ema):
        torch.manual_seed(0)
        vq = VectorQuantizer(a.codes, hidden, 0.25)
        vq.materialize_min_encodings = False
        model = Shelgon(a.model, vq, a.model, None, compute_dtype=torch.bfloat16).cuda()
        model.set_mode("full")
        return TrainEngine(model.train(), lr=1e-4, milestones=[10000, 20000], gamma=0.1, weight_ema=weight_ema)

    sync = torch.cuda.synchronize
    gen = torch.Generator().manual_seed(69)
    arms = {"off": build(None), "on": build(a.decay)}
    pools = {}
    for name, eng in arms.items():
        gen.manual_seed(69)
        pools[name] = [(ids.cuda(), mask.cuda()) for ids, mask in (random_token_batch(a.batch, a.seq, gen) for _ in range(8))]
        pools[name] = [(ids, mask, eng.pack_batch(ids, mask)) for ids, mask in pools[name]]

    def block(name, first, n):
        eng, pool = arms[name], pools[name]
        sync()
        t0 = time.perf_counter()
        for i in range(first, first + n):
            ids, mask, pack = pool[i % len(pool)]
            eng.train_step(ids, mask, prepared=pack)
        sync()
        return (time.perf_counter() - t0) / n * 1e3

    for name in arms:                                            # two eager steps, the capture, replays: every later step is a replay
        block(name, 0, 6)
    assert all(eng._graphs for eng in arms.values()), "the step was not captured"
    ms = {"off": [], "on": []}
    for b in range(a.blocks):
        for name in ("off", "on") if b % 2 == 0 else ("on", "off"):
            ms[name].append(block(name, 6 + b * a.steps, a.steps))
    nodes = {name: [c["kernel"] for c in next(iter(eng._graphs.values())).node_census()] for name, eng in arms.items()}

    # the kernels alone, over the whole flat buffer of the `on` engine, back to back on one stream between two events
    eng = arms["on"]
    fl = eng.flat
    lo, hi = max(fl.ranges, key=lambda r: r[1] - r[0])          # (mode full: the one range that covers the buffer)
    n = hi - lo

    def timed(fn):
        fn()
        sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_reps):
            fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1) / a.kernel_reps

    b1, b2 = eng.betas
    t_ema = timed(lambda: nnops.weight_ema_update(fl.master[lo:hi], fl.ema[lo:hi], eng._wema_state, a.decay))
    t_adam = timed(lambda: nnops.adam_step_dev(fl.master[lo:hi], fl.grad[lo:hi], fl.m[lo:hi], fl.v[lo:hi], eng._state, b1, b2, eng.eps,
                                               eng.wd, shadow=fl.shadow[lo:hi]))
    t_swap = timed(lambda: nnops.weight_ema_swap(fl.master[lo:hi], fl.ema[lo:hi], shadow=fl.shadow[lo:hi]))
    if (a.kernel_reps + 1) % 2:                                  # (warm-up + reps: an even count leaves the buffers where they were)
        nnops.weight_ema_swap(fl.master[lo:hi], fl.ema[lo:hi], shadow=fl.shadow[lo:hi])
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"shape": {"model": a.model, "batch": a.batch, "seq": a.seq, "codes": a.codes, "dtype": "bfloat16"},
           "params_flat": int(fl.n), "elements_updated": int(n), "ranges": len(fl.ranges), "decay": a.decay,
           "step_ms_off": ms["off"], "step_ms_on": ms["on"], "step_ms_off_median": med["off"], "step_ms_on_median": med["on"],
           "step_ms_added": med["on"] - med["off"], "steps_per_block": a.steps,
           "graph_kernel_nodes_off": nodes["off"], "graph_kernel_nodes_on": nodes["on"],
           "ema_update_ms": t_ema, "ema_update_bytes": 12 * n, "ema_update_tb_per_s": 12 * n / (t_ema * 1e-3) / 1e12,
           "adam_ms": t_adam, "adam_bytes": 28 * n, "adam_tb_per_s": 28 * n / (t_adam * 1e-3) / 1e12,
           "swap_ms": t_swap, "swap_bytes": 18 * n, "swap_tb_per_s": 18 * n / (t_swap * 1e-3) / 1e12,
           "weight_ema_updates": eng.weight_ema_updates, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
