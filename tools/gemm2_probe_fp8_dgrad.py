#!/usr/bin/env python3
"""Per input-gradient GEMM gx = gy . W of the step (8192 tokens): the own bf16 `nn` kernel against the fp8 path of
TrainEngine(fp8_backward=True) -- the e5m2 quantisation pass over gy, the fp8 NT GEMM on the transposed e4m3 weight, and that
weight's share of the per-step transpose -- which input gradients does fp8 pay for?  Last line: the segmented transpose over
every site of a 12 + 12 layer model, as the step launches it.
Every cell: median (minimum .. maximum) over `rounds` interleaved rounds of 20 launches between two events -- the spread says which
differences mean something; last column: the shader clock held while the row was measured (kvq_clock_probe).
usage: gemm2_probe_fp8_dgrad.py [rounds]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))
import torch  # noqa: E402
from kvq import nnops  # noqa: E402
from kvq._ffi import lib  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
dev, T = "cuda", 8192


def bench(fn, iters=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def rnd(*s, scale=1.0):
    return (torch.randn(s, device=dev) * scale).to(torch.bfloat16)


# (name, rows M of W = contraction, columns K of W = width of gx, accumulate into gx, launches per 12 + 12 layer step)
SITES = [("attention output / cross-q / head transform 768x768", 768, 768, False, 49), ("QKV 2304x768 (+=)", 2304, 768, True, 24),
         ("FFN1 3072x768 (+=)", 3072, 768, True, 24), ("FFN2 768x3072 (where not folded into the GELU' GEMM)", 768, 3072, False, 24),
         ("all-layer cross-K/V 18432x768", 18432, 768, False, 1)]
def cell(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:.1f} ({v[0]:.1f} .. {v[-1]:.1f})"


print("| input gradient (W rows x cols) | own bf16 nn us | e5m2 pass us | fp8 GEMM us | transpose of W us | fp8 total us (medians) | clock MHz |")
print("|---|---|---|---|---|---|---|")
for name, M, K, acc, _ in SITES:
    gy, W = rnd(T, M, scale=1e-3), rnd(M, K, scale=0.05)
    W8, sw = nnops.fp8_quantize(W)
    Wt8 = nnops.fp8_transpose(W8)
    st = torch.zeros(lib().kvq_fp8_state_floats(), dtype=torch.float32, device=dev)
    st[0] = 57344.0 / (4.0 * float(gy.float().abs().max()))
    g8 = nnops.fp8_quantize_delayed(gy, st, "e5m2")
    out = torch.zeros((T, K), device=dev, dtype=torch.bfloat16)
    fns = {"own": lambda: nnops.gemm(gy, W, "nn", out=out, accumulate=acc),
           "quant": lambda: nnops.fp8_quantize_delayed(gy, st, "e5m2", out=g8),
           "fp8": lambda: nnops.gemm_fp8_nt(g8, Wt8, st, sw, out=out, a_format="e5m2", accumulate=acc),
           "transpose": lambda: nnops.fp8_transpose(W8, out=Wt8)}
    res = {kk: [] for kk in fns}
    p0 = nnops.clock_probe()
    for _ in range(rounds):
        for kk in res:
            res[kk].append(bench(fns[kk]))
    p1 = nnops.clock_probe()
    torch.cuda.synchronize()
    mhz = nnops.clock_mhz(p0, p1)[0]
    med = {kk: sorted(v)[len(v) // 2] for kk, v in res.items()}
    tot = med["fp8"] + med["quant"] + med["transpose"]
    print(f"| {name} | {cell(res['own'])} | {cell(res['quant'])} | {cell(res['fp8'])} | {cell(res['transpose'])} | {tot:.1f} | {mhz:.0f} |", flush=True)

# the step's one segmented launch: 12 encoder layers (o, qkv, f1, f2), 12 decoder layers (+ cross o, q), cross-K/V, head transform
shapes = ([(768, 768), (2304, 768), (3072, 768), (768, 3072)] * 12 + [(768, 768), (2304, 768), (768, 768), (768, 768), (3072, 768), (768, 3072)] * 12
          + [(18432, 768), (768, 768)])
offs, o = [], 0
for r, c in shapes:
    offs.append(o)
    o += r * c
src = torch.randint(0, 256, (o,), device=dev, dtype=torch.int32).to(torch.uint8)
dst = torch.empty_like(src)
t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
tab = (t64(offs), t64([r for r, _ in shapes]), t64([c for _, c in shapes]), t64(offs))
tiles = max(-(-r // 128) * -(-c // 128) for r, c in shapes)
ts = sorted(bench(lambda: nnops.fp8_transpose_segments(src, dst, *tab, tiles)) for _ in range(rounds))
us = ts[len(ts) // 2]
print(f"\nsegmented transpose, {len(shapes)} weights, {o / 1e6:.1f} MB: {us:.1f} us ({ts[0]:.1f} .. {ts[-1]:.1f}) = {2 * o / us / 1e6:.2f} TB/s read + written")
