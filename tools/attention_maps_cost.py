"""What an attention-map census costs beside the forward it rides on (profiles/attention_maps.md).

    python tools/attention_maps_cost.py [--batch 256] [--seq 32] [--model kvq-bert-base-2l] [--calls 20] [--out FILE]

One Shelgon (VectorQuantizer, 9 codes) in bf16; three alternating windows of `--calls` calls each of TrainEngine.forward_logits and
TrainEngine.attention_maps(census=...) on the same batch, after a warm-up of both; every window between two device events.
Prints one JSON line: ms per call of each window, the medians, and the difference.  Needs the GPU (no fallback).

    python tools/attention_maps_cost.py --kernel [--runs 0,1,2,4,8]

times kvq_attn_probs alone (bf16, nh = 12, 32 x 32, causal with ragged masks, the engine's fused [N, 3H] layout) at B = 256 and
B = 2048, table only and table + per-sentence output, once per forced run length (KVQ_ATTN_PROBS_RUN, read once by the library:
one child process each; 0 = the library's rule): three windows of 200 launches each after a warm-up, median us per launch."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))

import torch  # noqa: E402


def kernel_child():
    """one process = one setting of KVQ_ATTN_PROBS_RUN: prints {shape: median us per launch}"""
    from kvq import nnops
    nh, S, H = 12, 32, 12 * 64
    res = {}
    for B in (256, 2048):
        g = torch.Generator().manual_seed(B)
        X = torch.randn(B * S, 3 * H, generator=g).bfloat16().cuda()
        lens = torch.randint(4, S + 1, (B,), generator=g)
        mask = (torch.arange(S)[None] < lens[:, None]).long().cuda()
        q, k, v = X[:, :H], X[:, H:2 * H], X[:, 2 * H:]
        table = torch.zeros(nh, S, S, dtype=torch.float64, device="cuda")
        probs = torch.empty(B, nh, S, S, device="cuda")
        for what, pr in (("table", None), ("table+probs", probs)):
            call = lambda: nnops.attn_probs(q, k, v, mask, B, nh, S, S, True, probs=pr, table=table)
            for _ in range(20):
                call()
            torch.cuda.synchronize()
            t = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(200):
                    call()
                e1.record()
                torch.cuda.synchronize()
                t.append(e0.elapsed_time(e1) * 1000 / 200)
            res[f"B{B} {what}"] = round(statistics.median(t), 2)
    print("KERNEL " + json.dumps(res))


def kernel_sweep(runs, out):
    import subprocess
    rows = {}
    for r in runs:
        env = dict(os.environ)
        env.pop("KVQ_ATTN_PROBS_RUN", None)
        if r > 0:
            env["KVQ_ATTN_PROBS_RUN"] = str(r)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-child"], env=env, capture_output=True, text=True, timeout=240)
        if p.returncode != 0:
            raise SystemExit(f"run length {r}: child failed\n{p.stdout[-2000:]}{p.stderr[-2000:]}")
        rows["rule" if r == 0 else f"run {r}"] = json.loads([l for l in p.stdout.splitlines() if l.startswith("KERNEL ")][-1][7:])
    line = json.dumps(dict(kernel_us_per_launch=rows, device=torch.cuda.get_device_name(0)))
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--kernel-child", action="store_true")
    ap.add_argument("--runs", default="0,1,2,4,8")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq", type=int, default=32)
    ap.add_argument("--model", default="kvq-bert-base-2l")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X")
    if a.kernel_child:
        return kernel_child()
    if a.kernel:
        return kernel_sweep([int(x) for x in a.runs.split(",")], a.out)
    from dsentences.synthetic import random_token_batch
    from kvq.census import AttentionCensus
    from kvq.engine import TrainEngine
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(0)
    vq = VectorQuantizer(9, 768, 0.1, vq_codebook_init_values=None)
    vq.materialize_min_encodings = False
    model = Shelgon(a.model, vq, a.model, None, compute_dtype=torch.bfloat16).cuda().eval()
    eng = TrainEngine(model)
    ids, mask = (t.cuda() for t in random_token_batch(a.batch, a.seq, torch.Generator().manual_seed(1), max_len=a.seq))
    census = AttentionCensus(eng.n_dec_layers, eng.nh, a.seq, a.seq)
    fwd = lambda: eng.forward_logits(ids, mask)
    maps = lambda: eng.attention_maps(ids, mask, census=census)

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    with torch.no_grad():
        for _ in range(5):
            fwd(); maps()
        torch.cuda.synchronize()
        t_fwd, t_maps = [], []
        for _ in range(3):
            t_fwd.append(window(fwd))
            t_maps.append(window(maps))
    res = dict(model=a.model, batch=a.batch, seq=a.seq, dtype="bfloat16", calls_per_window=a.calls,
               forward_logits_ms=[round(t, 4) for t in t_fwd], attention_maps_ms=[round(t, 4) for t in t_maps],
               forward_logits_median_ms=round(statistics.median(t_fwd), 4), attention_maps_median_ms=round(statistics.median(t_maps), 4),
               sentences_in_census=census.count, device=torch.cuda.get_device_name(0))
    res["extra_ms"] = round(res["attention_maps_median_ms"] - res["forward_logits_median_ms"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
