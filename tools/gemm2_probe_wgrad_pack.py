#!/usr/bin/env python3
"""The packed weight-gradient launches against the ones they replace (TN, contraction over 8192 tokens), on rotating (cold) operand
sets, the arms interleaved in every round; us per launch as median [min .. max] over the rounds.
  * LM head [30528, 768]: one 128 x 256 launch (the unpacked schedule) / the mixed launch (a full round of 256 x 256 tiles, the rest
    on 128 x 256 tiles), alone -- what the step runs -- and with head.t.w in its short round;
  * either tile class through the mixed kernel against its single-shape kernel (does the shared register allocation cost?);
  * an encoder pair (216 tiles of 256 x 256) with and without two cross-K/V slices (252 tiles), a decoder pair (252) with and
    without a 256-row slice of head.t.w (255): what the riders cost the launch that takes them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))
import torch  # noqa: E402
from kvq import nnops  # noqa: E402

T, H, VP, dev = 8192, 768, 30528, "cuda"
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
rnd = lambda *s: torch.randn(s, device=dev).to(torch.bfloat16)  # noqa: E731
ENC = [(2304, 768), (768, 768), (3072, 768), (768, 3072)]
DEC = ENC + [(768, 768), (768, 768)]
N_CU = torch.cuda.get_device_properties(0).multi_processor_count


def make(shapes):
    keep = [(rnd(T, m), rnd(T, n), torch.empty((m, n), device=dev, dtype=torch.bfloat16)) for m, n in shapes]
    return [nnops.gemm_problem(g, x, o, "tn") for g, x, o in keep], keep


def make_head():
    """[LM head on rows [0, r), rows [r, VP), head.t.w], the whole LM head as one problem."""
    g, x, o = rnd(T, VP), rnd(T, H), torch.empty((VP, H), device=dev, dtype=torch.bfloat16)
    r = N_CU // 3 * 256
    t, keep = make([(H, H)])
    split = [nnops.gemm_problem(g[:, :r], x, o[:r], "tn"), nnops.gemm_problem(g[:, r:], x, o[r:], "tn")] + t
    return split, (g, x, o), keep


def make_pair_with_slices():
    """an encoder pair, and the same with two per-layer slices of the all-layer cross-K/V gradient [18432, 768]"""
    pair, keep = make(ENC * 2)
    g, x, o = rnd(T, 24 * H), rnd(T, H), torch.empty((24 * H, H), device=dev, dtype=torch.bfloat16)
    sl = [nnops.gemm_problem(g[:, i * 2 * H:(i + 1) * 2 * H], x, o[i * 2 * H:(i + 1) * 2 * H], "tn") for i in (3, 8)]
    return pair, pair + sl, (keep, g, x, o)


head = [make_head() for _ in range(2)]
pairs = [make_pair_with_slices() for _ in range(4)]
decs = [make(DEC * 2) for _ in range(4)]
decs_t = [make(DEC * 2 + [(256, 768)]) for _ in range(4)]        # + one 256-row slice of head.t.w
encs = [make(ENC) for _ in range(6)]
MIXED3 = ["256x256", "128x256", "128x256"]
ARMS = {
    "LM head, one 128x256 launch (717 tiles)": [lambda h=h: nnops.gemm(h[1][0], h[1][1], "tn", out=h[1][2], tile="128x256") for h in head],
    "LM head + head.t.w, mixed (255 + 225)": [lambda h=h: nnops.gemm_grouped_mixed(h[0], MIXED3) for h in head],
    "LM head alone, mixed (255 + 207)": [lambda h=h: nnops.gemm_grouped_mixed(h[0][:2], MIXED3[:2]) for h in head],
    "2 dec layers 256x256, grouped (252)": [lambda d=d: nnops.gemm_grouped(d[0], "tn", "256x256") for d in decs],
    "2 dec layers 256x256, mixed kernel (252)": [lambda d=d: nnops.gemm_grouped_mixed(d[0], ["256x256"] * len(d[0])) for d in decs],
    "2 dec layers + a head.t.w slice (255)": [lambda d=d: nnops.gemm_grouped(d[0], "tn", "256x256") for d in decs_t],
    "1 enc layer 128x256, grouped (216)": [lambda e=e: nnops.gemm_grouped(e[0], "tn", "128x256") for e in encs],
    "1 enc layer 128x256, mixed kernel (216)": [lambda e=e: nnops.gemm_grouped_mixed(e[0], ["128x256"] * len(e[0])) for e in encs],
    "enc pair (216)": [lambda p=p: nnops.gemm_grouped(p[0], "tn", "256x256") for p in pairs],
    "enc pair + 2 cross-K/V slices (252)": [lambda p=p: nnops.gemm_grouped(p[1], "tn", "256x256") for p in pairs],
}

# the mixed launch stores what the single-shape launches store
ref = torch.empty_like(head[0][1][2])
nnops.gemm(head[0][1][0], head[0][1][1], "tn", out=ref, tile="128x256")
ARMS["LM head + head.t.w, mixed (255 + 225)"][0]()
torch.cuda.synchronize()
r = N_CU // 3 * 256
assert torch.equal(ref[r:], head[0][1][2][r:]), "128 x 256 rows differ from the single-shape launch"
want = head[0][1][0].float().t()[:512] @ head[0][1][1].float()
assert ((head[0][1][2][:512].float() - want).norm() / want.norm()).item() < 5e-3

times = {k: [] for k in ARMS}
for rd in range(ROUNDS + 1):                        # round 0 warms up
    for name, calls in ARMS.items():
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for c in calls:
            c()
        e1.record()
        torch.cuda.synchronize()
        if rd:
            times[name].append(e0.elapsed_time(e1) / len(calls) * 1e3)
print(f"{N_CU} CUs, {ROUNDS} interleaved rounds, us per launch: median [min .. max]")
for name, ts in times.items():
    s = sorted(ts)
    print(f"{name:44s} {s[len(s) // 2]:7.1f} [{s[0]:7.1f} .. {s[-1]:7.1f}]", flush=True)
