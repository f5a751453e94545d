"""LayerNorm launch time of two (or more) builds of libkvq.so against each other: `python tools/ln_cost_libs.py PARENT_LIB TREE_LIB
[MORE_LIBS ...] [--out FILE.json]`.  All libraries loaded into ONE process, every arm on preallocated buffers straight through the
C entry points (no allocation between launches), bf16, p_drop = 0.1:

  ln_fwd            kvq_dropout_residual_ln_fwd with a residual            [8192, 768]
  ln_fwd_nores      the same without one (the LayerNorm-only pass)         [8192, 768]
  ln_fwd_fp8        kvq_dropout_residual_ln_fwd_fp8                        [8192, 768]
  embed_ln_fwd      kvq_embed_ln_fwd (V = 30522, S = 32)                   [8192, 768]
  ln_bwd            kvq_dropout_residual_ln_bwd_partial, want_dbias = 1    [8192, 768]   (drln_bwd16_kernel<3>)
  ln_dropout_bwd    kvq_ln_dropout_bwd_partial                             [8192, 768]   (drln_bwd16_kernel<3>, drop_on_out)
  ln_bwd_3072       kvq_dropout_residual_ln_bwd_partial, want_dbias = 1    [8192, 3072]  (drln_bwd_kernel<bf16, 16>)

After a warm-up, --rounds rounds; in every round each arm runs one window per library, the libraries alternating, each window at
least --window-s long between two device events.  The bar of an arm, for every library after the first: its median lies inside
the first library's own min - max over its rounds of that arm.  Prints one JSON line (microseconds per launch)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.3)
    a = ap.parse_args()
    if not torch.cuda.is_available() or len(a.libs) < 2:
        raise SystemExit("ln_cost_libs.py needs an MI355X and at least two libraries")
    from kvq import _ffi

    libs = []
    for path in a.libs:
        lib = ctypes.CDLL(os.path.abspath(path))
        for name, (res, args) in _ffi.SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        libs.append(lib)

    N, EPS, P, SEED, SITE, BF = 8192, 1e-12, 0.1, 3, 4, _ffi.KVQ_BF16
    torch.manual_seed(0)
    st = _ffi.stream_ptr()
    keep = []                                                      # every buffer lives until the end

    def buf(*shape, dtype=torch.bfloat16, rand=True):
        t = torch.randn(*shape, device="cuda").to(dtype) if rand else torch.empty(*shape, device="cuda", dtype=dtype)
        keep.append(t)
        return t.data_ptr()

    def shape_arms(H, tag, forward):
        y, r, g, out, pre, gy, gr = (buf(N, H) for _ in range(7))
        gamma, beta = buf(H, dtype=torch.float32), buf(H, dtype=torch.float32)
        mean, rstd = buf(N, dtype=torch.float32, rand=False), buf(N, dtype=torch.float32, rand=False)
        nbytes = libs[0].kvq_ln_bwd_workspace_bytes(N, H)
        part = buf(nbytes, dtype=torch.uint8, rand=False)
        libs[0].kvq_dropout_residual_ln_fwd(y, r, gamma, beta, N, H, EPS, P, SEED, SITE, BF, out, pre, mean, rstd, st)   # pre, mean, rstd of the backward arms
        arms = {
            "ln_bwd" + tag: lambda lib: lib.kvq_dropout_residual_ln_bwd_partial(g, pre, mean, rstd, gamma, N, H, P, SEED, SITE, BF, gy, gr, 1, part, nbytes, st),
        }
        if forward:
            out2, pre2 = buf(N, H), buf(N, H)
            out8 = buf(N, H, dtype=torch.uint8, rand=False)
            state = torch.zeros(libs[0].kvq_fp8_state_floats(), device="cuda")
            state[0] = 37.0
            keep.append(state)
            V, S = 30522, 32
            ids = torch.randint(0, V, (N,), device="cuda")
            keep.append(ids)
            word, pos, typ = buf(V, H), buf(S, H), buf(1, H)
            arms.update({
                "ln_fwd": lambda lib: lib.kvq_dropout_residual_ln_fwd(y, r, gamma, beta, N, H, EPS, P, SEED, SITE, BF, out2, pre2, mean, rstd, st),
                "ln_fwd_nores": lambda lib: lib.kvq_dropout_residual_ln_fwd(y, None, gamma, beta, N, H, EPS, P, SEED, SITE, BF, out2, pre2, mean, rstd, st),
                "ln_fwd_fp8": lambda lib: lib.kvq_dropout_residual_ln_fwd_fp8(y, r, gamma, beta, N, H, EPS, P, SEED, SITE, out2, pre2, mean, rstd, out8,
                                                                               state.data_ptr(), st),
                "embed_ln_fwd": lambda lib: lib.kvq_embed_ln_fwd(ids.data_ptr(), word, pos, typ, gamma, beta, N, S, H, V, EPS, P, SEED, SITE, BF, out2,
                                                                   pre2, mean, rstd, st),
                "ln_dropout_bwd": lambda lib: lib.kvq_ln_dropout_bwd_partial(g, pre, mean, rstd, gamma, N, H, P, SEED, SITE, BF, gy, part, nbytes, st),
            })
        return arms

    arms = {**shape_arms(768, "", True), **shape_arms(3072, "_3072", False)}
    names = ("ln_fwd", "ln_fwd_nores", "ln_fwd_fp8", "embed_ln_fwd", "ln_bwd", "ln_dropout_bwd", "ln_bwd_3072")
    torch.cuda.synchronize()

    def window(lib, fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            if fn(lib) != 0:
                raise SystemExit("a launch failed: " + (lib.kvq_last_error() or b"?").decode())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps * 1e3

    reps = {}
    for k in names:                                                # warm-up, and the launch count that fills a window
        for lib in libs:
            window(lib, arms[k], 50)
        reps[k] = max(50, int(a.window_s * 1e6 / window(libs[0], arms[k], 200)) + 1)
    us = [{k: [] for k in names} for _ in libs]
    for _ in range(a.rounds):
        for k in names:
            for i, lib in enumerate(libs):
                us[i][k].append(window(lib, arms[k], reps[k]))
    med = [{k: statistics.median(v) for k, v in m.items()} for m in us]
    lo, hi = {k: min(us[0][k]) for k in names}, {k: max(us[0][k]) for k in names}
    res = {"shape": {k: [N, 3072 if k.endswith("_3072") else 768] for k in names}, "launches_per_window": reps, "rounds": a.rounds, "libs": a.libs, "us": us, "us_median": med,
           "first_lib_min_us": lo, "first_lib_max_us": hi,
           "median_not_above_first_lib_max": [{k: med[i][k] <= hi[k] for k in names} for i in range(1, len(libs))],
           "median_inside_first_lib_min_max": [{k: lo[k] <= med[i][k] <= hi[k] for k in names} for i in range(1, len(libs))],
           "vs_first_pct": [{k: (med[i][k] / med[0][k] - 1) * 100 for k in names} for i in range(1, len(libs))],
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
