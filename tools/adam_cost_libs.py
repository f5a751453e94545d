"""Adam launch time of two (or more) builds of libkvq.so against each other: `python tools/adam_cost_libs.py PARENT_LIB TREE_LIB
[MORE_LIBS ...] [--out FILE.json]`.  The arms of tools/adam_groups_cost.py at the benchmarked flat length (bert-base-uncased, bf16
gradient, bf16 shadow, mode full) and an fp8-mirror arm, all libraries loaded into ONE process:

  a, a2  kvq_adam_step_dev                                        b  kvq_adam_step_grouped, one group
  c      kvq_adam_step_grouped with the engine's block table      d  arm b with decoupled = 1
  f      kvq_adam_step_dev_fp8 on the buffers of an fp8 engine (its mirror, span table and scales)

After a warm-up, --rounds rounds of a, b, a2, c, d, f; in every round each arm runs one window per library, the libraries
alternating, each window at least --window-s long between two device events.  The bar of an arm, for every library after the first:
its median may exceed the first library's median by no more than the first library's own spread -- the largest difference between
its rounds of that arm plus the difference between the medians of its two a-arms.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))

import torch  # noqa: E402

ARMS = ("a", "b", "a2", "c", "d", "f")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", default="bert-base-uncased")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available() or len(a.libs) < 2:
        raise SystemExit("adam_cost_libs.py needs an MI355X and at least two libraries")
    from kvq import _ffi, nnops
    from kvq.engine import NO_DECAY, TrainEngine
    from models.bagon.Bagon import LOCAL_BERT_CONFIGS
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer

    def engine(**kw):
        torch.manual_seed(0)
        vq = VectorQuantizer(512, LOCAL_BERT_CONFIGS[a.model].get("hidden_size", 768), 0.25)
        vq.materialize_min_encodings = False
        model = Shelgon(a.model, vq, a.model, None, compute_dtype=torch.bfloat16).cuda()
        model.set_mode("full")
        eng = TrainEngine(model.train(), lr=1e-4, weight_decay=0.01, **kw)
        fl = eng.flat
        lo, hi = max(fl.ranges, key=lambda r: r[1] - r[0])        # (mode full: the one range that covers the buffer)
        fl.grad.normal_(0.0, 1e-3)                                 # a gradient that is not all zeros; lr = 1e-4 keeps the weights finite
        nnops.step_state_advance(eng._state, eng.lr, eng.gamma, [], *eng.betas)
        views = (fl.master[lo:hi], fl.grad[lo:hi], fl.m[lo:hi], fl.v[lo:hi], eng._state, *eng.betas, eng.eps, eng.wd)
        return eng, views, fl.shadow[lo:hi], lo

    geng, gv, gsh, glo = engine(param_groups=[{"match": NO_DECAY, "weight_decay": 0.0}])
    feng, fv, fsh, flo = engine(fp8_forward=True)
    pg = geng._pg
    one = dict(group_lr_scale=pg["scale"][:1], group_wd=pg["wd"][:1], n_groups=1)
    arms = {
        "a": lambda: nnops.adam_step_dev(*gv, shadow=gsh),
        "b": lambda: nnops.adam_step_grouped(*gv, shadow=gsh, **one),
        "c": lambda: nnops.adam_step_grouped(*gv, shadow=gsh, block_group=pg["blocks"], first_element=glo, group_lr_scale=pg["scale"],
                                             group_wd=pg["wd"], n_groups=len(pg["table"])),
        "d": lambda: nnops.adam_step_grouped(*gv, shadow=gsh, decoupled=True, **one),
        "f": lambda: nnops.adam_step_dev(*fv, shadow=fsh, fp8=(*feng._w8_adam, flo)),
    }
    arms["a2"] = arms["a"]
    libs = []
    for path in a.libs:                                            # (kvq._ffi.lib() hands out the one set in window())
        lib = ctypes.CDLL(os.path.abspath(path))
        for name, (res, args) in _ffi.SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        libs.append(lib)

    def window(lib, fn, reps):
        _ffi._lib = lib
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    for lib in libs:                                               # warm-up, and the launch count that fills a window
        for fn in arms.values():
            window(lib, fn, 20)
    reps = max(20, int(a.window_s * 1e3 / window(libs[0], arms["a"], 50)) + 1)
    ms = [{k: [] for k in ARMS} for _ in libs]
    for _ in range(a.rounds):
        for k in ARMS:
            for i, lib in enumerate(libs):
                ms[i][k].append(window(lib, arms[k], reps))
    med = [{k: statistics.median(v) for k, v in m.items()} for m in ms]
    aa = abs(med[0]["a"] - med[0]["a2"])
    bar = {k: med[0][k] + (max(ms[0][k]) - min(ms[0][k])) + aa for k in ARMS}
    res = {"model": a.model, "elements": int(gv[0].numel()), "launches_per_window": reps, "rounds": a.rounds, "libs": a.libs, "ms": ms,
           "ms_median": med, "first_lib_a_vs_a2_ms": aa, "bar_ms": bar,
           "within_bar": [{k: med[i][k] <= bar[k] for k in ARMS} for i in range(1, len(libs))],
           "vs_first_pct": [{k: (med[i][k] / med[0][k] - 1) * 100 for k in ARMS} for i in range(1, len(libs))],
           "finite": bool(torch.isfinite(gv[0]).all() and torch.isfinite(fv[0]).all()), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
