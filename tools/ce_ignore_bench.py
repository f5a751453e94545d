"""The loss kernels against their ignore_index twins at the benchmarked shape: N = 8192 rows, V = 30522, ld = 30528, bf16, targets of
dsentences.synthetic.random_token_batch(256, 32) (4 - 12 real tokens per sentence, pad id 0).  Launches each kernel REPS times on
its own copy of the logits (the backward runs in place, as the engine's does; the copy is restored before every launch by a
copy kernel the trace lists separately).  Meant to run under `rocprofv3 --kernel-trace --stats -- python tools/ce_ignore_bench.py`;
without the profiler it prints device-event times (one event pair around each launch) as a cross-check.  Bytes from the shape:
forward reads N * V elements, backward reads N * V and writes N * ld; the twins read only the counted rows."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kindergarten-vq-vae_amd"))
from dsentences.synthetic import random_token_batch  # noqa: E402
from kvq._ffi import check, lib, stream_ptr  # noqa: E402

REPS = int(os.environ.get("REPS", "20"))
B, S, V, LD, PAD = 256, 32, 30522, 30528, 0
N = B * S
dev = "cuda"
ids, _ = random_token_batch(B, S, torch.Generator().manual_seed(0))
tgt = ids.reshape(-1).to(dev)
counted = int((tgt != PAD).sum())
src = (torch.randn(N, LD, device=dev) * 2).bfloat16()
work = torch.empty_like(src)
rl = torch.empty(N, device=dev); lse = torch.empty(N, device=dev); pred = torch.empty(N, dtype=torch.int64, device=dev)
out = torch.zeros(3, device=dev)
g = torch.ones(1, device=dev)
P = lib().kvq_ce_bwd_partial_rows(N)
part = torch.empty(P, LD, device=dev)
L = lib()

calls = {
    "kvq_ce_forward": lambda: check(L.kvq_ce_forward(work.data_ptr(), tgt.data_ptr(), N, V, LD, 1, rl.data_ptr(), lse.data_ptr(), pred.data_ptr(),
                                                     out[0:].data_ptr(), out[1:].data_ptr(), stream_ptr()), "fwd"),
    "kvq_ce_forward_ignore": lambda: check(L.kvq_ce_forward_ignore(work.data_ptr(), tgt.data_ptr(), N, V, LD, 1, PAD, rl.data_ptr(), lse.data_ptr(),
                                                                   pred.data_ptr(), out[0:].data_ptr(), out[1:].data_ptr(), out[2:].data_ptr(),
                                                                   stream_ptr()), "fwd_ignore"),
    "kvq_ce_backward_bias": lambda: check(L.kvq_ce_backward_bias(work.data_ptr(), tgt.data_ptr(), lse.data_ptr(), g.data_ptr(), N, V, LD, 1,
                                                                 work.data_ptr(), part.data_ptr(), part.numel() * 4, stream_ptr()), "bwd"),
    "kvq_ce_backward_bias_ignore": lambda: check(L.kvq_ce_backward_bias_ignore(work.data_ptr(), tgt.data_ptr(), lse.data_ptr(), g.data_ptr(),
                                                                               out[2:].data_ptr(), PAD, N, V, LD, 1, work.data_ptr(), part.data_ptr(),
                                                                               part.numel() * 4, stream_ptr()), "bwd_ignore"),
}
print(f"N {N} V {V} ld {LD} bf16: {counted} of {N} rows counted ({100.0 * (N - counted) / N:.1f} % pad), {REPS} launches each")
for name, fn in calls.items():
    if "backward" in name:                      # lse (and count) of the matching forward
        work.copy_(src)
        calls["kvq_ce_forward_ignore" if name.endswith("ignore") else "kvq_ce_forward"]()
    ms = []
    for r in range(REPS + 3):
        work.copy_(src)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        if r >= 3:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    print(f"{name}: median {ms[len(ms) // 2] * 1e3:.1f} us, min {ms[0] * 1e3:.1f} us (device events, finalize launch included)")
