"""Two builds of libkvq.so against each other on the Adam family and the step state of csrc/kvq_adam.hip: `python
tools/adam_compare_libs.py LIB_A LIB_B`.  Both libraries are loaded into this one process and run on the same seeded inputs, every
buffer a view inside a frame of sentinels (tests/test_adam_parity_gpu.py: framed); every output must be equal BY BITS, its frame
included: p, m, v, vmax, the bf16 shadow, the fp8 mirror, the gradient (an input no launch may touch) and the step state.

  kvq_adam_step, _dev, _guarded          tests/_adam_ref.covering_cases() (the guard's coefficient 0.37; grad_scale 1, 1 / 3, 1024)
  kvq_adam_step_dev_fp8, _guarded_fp8    the hyper-parameters of each covering case on the mirror layout of
                                         test_fp8_mirror_combinations (these entries take multiples of 8 elements: the launch starts
                                         at element 1032 and crosses spans of all three kinds)
  kvq_adam_step_grouped, _guarded        the launches of tests/test_adam_groups_kernels_gpu.py: the table form (launches(): 2 and
                                         16 groups, first elements 0, 16, 4112) and the one-group form (NS), coupled and decoupled
  kvq_step_state_advance, _sched         steps 1 .. 12 without and with milestones [3, 8], all three decay kinds, as raw words

One line per comparison; the first difference ends the run with exit status 1."""
import ctypes
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _adam_ref as R  # noqa: E402
import test_adam_groups_kernels_gpu as TG  # noqa: E402
import test_adam_parity_gpu as T  # noqa: E402
from kvq import _ffi, nnops  # noqa: E402
from kvq.engine import fp8_span_table  # noqa: E402

COEF = 0.37
lines = {}


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _ffi.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def compare(name, what, run):
    """run() -> {output name: tensor} under each library in turn (kvq._ffi.lib() hands out the one set here)."""
    res = []
    for lib in LIBS:
        _ffi._lib = lib
        res.append(run())
        torch.cuda.synchronize()
    a, b = res
    for k in a:
        wa, wb = a[k].view(torch.uint8), b[k].view(torch.uint8)
        if not torch.equal(wa, wb):
            diff = (wa != wb).nonzero()
            sys.exit(f"{name} {what}: DIFFERENT {k}: {len(diff)} of {wa.numel()} bytes, the first at {int(diff[0])}")
    lines[name] = lines.get(name, 0) + 1
    print(f"{name} {what}: equal ({', '.join(f'{k} {a[k].numel()}' for k in a)})")


def frames_of(x, n):
    fr = {k: T.framed(x[k]) for k in ("p", "m", "v", "vmax", "g") if x[k] is not None}
    fr["shadow"] = T.framed(n=n, dtype=T.BF16)
    return fr, (lambda k: fr[k][1] if k in fr else None)


def wholes(fr, **more):
    return {**{k + "_framed": w for k, (w, _) in fr.items()}, **more}


def plain(c, entry):
    def run():
        fr, v = frames_of(R.case_inputs(c), c.n)
        kw = dict(beta1=c.betas[0], beta2=c.betas[1], eps=R.ADAM_EPS, weight_decay=c.wd, vmax=v("vmax"), shadow=v("shadow"),
                  grad_scale=c.grad_scale)
        if entry == "kvq_adam_step":
            nnops.adam_step(v("p"), v("g"), v("m"), v("v"), c.t, R.LR, **kw)
            return wholes(fr)
        st = T.state_at(nnops, c.t, R.LR, *c.betas)
        nnops.adam_step_dev(v("p"), v("g"), v("m"), v("v"), st, guard=T.guard_with(nnops, COEF) if "guarded" in entry else None, **kw)
        return wholes(fr, step_state=st)
    compare(entry, T.case_name(c), run)


def mirror(c, entry):
    total, first = 6 * T.SPAN, 1032
    n = total - first - 40
    segs = [(T.SPAN + 16, 1024), (2 * T.SPAN, 2 * T.SPAN), (5 * T.SPAN + 512, 512)]
    c = c._replace(n=n)

    def run():
        fr, v = frames_of(R.case_inputs(c), n)
        fr["w8"] = T.framed(n=total, dtype=torch.uint8)
        off, cnt = (torch.tensor([s[i] for s in segs], dtype=torch.int64, device="cuda") for i in (0, 1))
        scale = torch.tensor([300.0, 2000.0, 900.0], device="cuda")
        span = torch.from_numpy(fp8_span_table(off.tolist(), cnt.tolist(), total, T.SPAN)).cuda()
        st = T.state_at(nnops, c.t, R.LR, *c.betas)
        nnops.adam_step_dev(v("p"), v("g"), v("m"), v("v"), st, beta1=c.betas[0], beta2=c.betas[1], eps=R.ADAM_EPS, weight_decay=c.wd,
                            vmax=v("vmax"), shadow=v("shadow"), grad_scale=c.grad_scale,
                            guard=T.guard_with(nnops, COEF) if "guarded" in entry else None, fp8=(v("w8"), span, scale, off, cnt, len(segs), first))
        torch.cuda.synchronize()                                       # (the tables live until here)
        return wholes(fr, step_state=st)
    compare(entry, T.case_name(c), run)


def grouped(c, what, blocks, first, scale, wd, decoupled, guarded):
    entry = "kvq_adam_step_grouped" + "_guarded" * guarded

    def run():
        fr, v = frames_of(R.case_inputs(c), c.n)
        st = T.state_at(nnops, c.t, R.LR, *c.betas)
        nnops.adam_step_grouped(v("p"), v("g"), v("m"), v("v"), st, beta1=c.betas[0], beta2=c.betas[1], eps=R.ADAM_EPS, weight_decay=c.wd,
                                vmax=v("vmax"), shadow=v("shadow"), grad_scale=c.grad_scale,
                                guard=T.guard_with(nnops, COEF) if guarded else None,
                                block_group=blocks.cuda() if blocks is not None else None, first_element=first,
                                group_lr_scale=torch.tensor(scale, device="cuda"), group_wd=torch.tensor(wd, device="cuda"),
                                n_groups=len(scale), decoupled=decoupled)
        return wholes(fr, step_state=st)
    compare(entry, f"{what} {'decoupled' if decoupled else 'coupled'}, {T.case_name(c)}", run)


def step_state(t, milestones, kind):
    def run(sched):
        whole, st = T.framed(n=3, dtype=torch.int64)
        st.copy_(torch.tensor([t - 1, 0, T.PAD_WORD << 32], dtype=torch.int64))
        if sched:
            nnops.step_state_advance_sched(st, TG.LR0, TG.GAMMA_LR, milestones, 0.9, 0.999, warmup_steps=TG.W, decay_kind=kind,
                                           total_steps=TG.T if kind else 0, min_ratio=0.1)
        else:
            nnops.step_state_advance(st, TG.LR0, TG.GAMMA_LR, milestones, 0.9, 0.999)
        return dict(step_state_framed=whole)
    compare("kvq_step_state_advance_sched", f"t = {t}, milestones {milestones}, kind {kind}", lambda: run(True))
    if kind == 0:
        compare("kvq_step_state_advance", f"t = {t}, milestones {milestones}", lambda: run(False))


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    LIBS = [load(p) for p in sys.argv[1:]]
    for c in R.covering_cases():
        for entry in ("kvq_adam_step", "kvq_adam_step_dev", "kvq_adam_step_guarded"):
            plain(c, entry)
        for entry in ("kvq_adam_step_dev_fp8", "kvq_adam_step_guarded_fp8"):
            mirror(c, entry)
    for decoupled in (False, True):
        for guarded in (False, True):
            for c, first, ng in TG.launches():
                grouped(c, f"table of {ng} groups, first {first},", TG.block_table(c.n, first, ng), first, *TG.TABLES[ng], decoupled, guarded)
            for i, n in enumerate(TG.NS):
                c = R.Case(n=n, gdtype=(T.F32, T.BF16)[i % 2], amsgrad=bool(i % 2), wd=0.3, grad_scale=1.0 / 3.0, betas=(0.9, 0.999), t=3,
                           seed=600 + i)
                grouped(c, "one group,", None, 0, [10.0], [0.01], decoupled, guarded)
    for t in range(1, 13):
        for milestones in ([], [3, 8]):
            for kind in (0, 1, 2):
                step_state(t, milestones, kind)
    print(f"{sys.argv[1]} and {sys.argv[2]}: {sum(lines.values())} comparisons, every output equal by bits (" +
          ", ".join(f"{n} {c}" for n, c in lines.items()) + ")")
