"""CPU self-check of tests/_adam_groups_ref.py: the f64 reference is torch.optim.Adam / AdamW with param groups, sched_ref is torch's
LinearLR / CosineAnnealingLR phase by phase, and the judges accept an op-by-op numpy float32 restatement of the grouped contract
(include/kvq.h "parameter groups") on the full input generator and reject each planted mistake on the same inputs.

A judge that counts roundings cannot tell two orders of the same operations apart: fl(fl(lr / bc1) * s_j) and fl(fl(lr * s_j) / bc1)
both sit inside GAMMA(9).  The planted "scale behind the division by bc1" mistakes are therefore the two ways in which taking the
scale out of lr_j and applying it to u goes wrong in value: the scale dividing (lr / (bc1 * s_j)), and -- decoupled -- the decay
factor left with the unscaled rate."""
import math

import numpy as np
import pytest
import torch

import _adam_groups_ref as G
import _adam_ref as R

F = np.float32
SCALES = [1.0, 0.1, 10.0, 0.0]
DECAYS = [0.01, 0.0, 0.01, 0.01]
N = R.ALL3
FIRST = 4096 + 16


def tables(n=N, first=FIRST):
    """A block table that changes group at every block, inside a larger one whose other entries hold an out-of-range id."""
    nb = (first + n + 15) // 16 + 4
    blocks = torch.full((nb,), 0xEE, dtype=torch.uint8)
    lo, hi = first // 16, (first + n + 15) // 16
    blocks[lo:hi] = (torch.arange(hi - lo) % len(SCALES)).to(torch.uint8)
    return blocks


def restate(x, c, blocks, first, decoupled, coef=None, mistake=None):
    """adam_group_kernel in numpy float32, one rounding per operation, in the kernel's order; `mistake` plants one deviation."""
    lr, b1, b2, eps, gs = (F(z) for z in (R.LR, c.betas[0], c.betas[1], R.ADAM_EPS, c.grad_scale))
    if coef is not None:
        gs = gs * F(coef)
    hp = R.case_hyper(c, coef)
    bc1, bc2s = F(hp.bc1), F(hp.bc2s)
    grp = G.element_groups(blocks, first + (16 if mistake == "group table shifted by one block" else 0), c.n).numpy()
    grp = grp % len(SCALES)                                   # (the shifted table reads one poisoned entry behind the launch's own)
    s, wd = np.array(SCALES, dtype=F)[grp], np.array(DECAYS, dtype=F)[grp]
    p, m, v = (x[k].numpy().copy() for k in ("p", "m", "v"))
    g = x["g"].float().numpy()
    one = F(1.0)
    with np.errstate(all="ignore"):
        lr_j = lr * s
        if mistake == "scale divides behind the division by bc1":
            lr_j = lr
        gv = g * gs
        if decoupled:
            keep = one - (lr if mistake == "decay factor with the unscaled rate" else lr_j) * wd
            p = p * keep
            if mistake == "decoupled decay that also feeds m":
                gv = gv + p * wd
        else:
            gv = gv + p * wd
        m1 = m * b1 + gv * (one - b1)
        v1 = v * b2 + (gv * gv) * (one - b2)
        d, vm1 = v1, None
        if c.amsgrad:
            vm1 = np.maximum(x["vmax"].numpy(), v1)
            d = vm1
        den = np.sqrt(d) / bc2s + eps
        step = lr_j / bc1
        if mistake == "scale divides behind the division by bc1":
            step = np.where(s > 0, lr / (bc1 * np.where(s > 0, s, one)), F(0.0)).astype(F)
        if mistake == "decay factor with the unscaled rate":
            step = (lr / bc1) * s
        p1 = p - step * (m1 / den)
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    t = torch.from_numpy
    return dict(p=t(p1), m=t(m1), v=t(v1), vmax=t(vm1) if vm1 is not None else None)


def judge(out, x, c, blocks, first, decoupled, coef=None):
    s_e, wd_e = G.element_tables(G.element_groups(blocks, first, c.n), SCALES, DECAYS)
    return {k: float(r.max()) for k, r in G.grouped_ratios(out, x, R.case_hyper(c, coef), s_e, wd_e, decoupled).items()}


CASES = [c for c in R.covering_cases() if c.n == N]
MISTAKES = {      # mistake -> (the decoupled values it exists for, the judged output it must push past 1)
    "scale divides behind the division by bc1": ((False, True), "p"),
    "decay factor with the unscaled rate": ((True,), "p"),
    "decoupled decay that also feeds m": ((True,), "m"),
    "group table shifted by one block": ((False, True), "p"),
}


@pytest.mark.parametrize("decoupled", [False, True])
def test_judges_accept_the_restated_contract(decoupled):
    assert len(CASES) >= 8
    worst = {}
    for i, c in enumerate(CASES):
        x, blocks = R.case_inputs(c), tables()
        coef = (None, 0.37)[i % 2]
        for k, w in judge(restate(x, c, blocks, FIRST, decoupled, coef), x, c, blocks, FIRST, decoupled, coef).items():
            worst[k] = max(w, worst.get(k, 0.0))
    print("FIGURE restated contract, decoupled", decoupled, {k: round(w, 4) for k, w in worst.items()})
    assert set(worst) == {"m", "v", "vmax", "p"} and max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_judges_reject_planted_mistakes(mistake):
    arms, what = MISTAKES[mistake]
    for decoupled in arms:
        for c in CASES:
            x, blocks = R.case_inputs(c), tables()
            w = judge(restate(x, c, blocks, FIRST, decoupled, mistake=mistake), x, c, blocks, FIRST, decoupled)
            assert w[what] > 1.0, f"'{mistake}' passes the {what} judge (decoupled {decoupled}, {c}): {w}"


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("amsgrad", [False, True])
def test_reference_is_torch_adam_with_param_groups(decoupled, amsgrad):
    """grouped_ref iterated over 5 steps against torch.optim.Adam / AdamW with one param group per table entry, f64: 1e-12."""
    gen = torch.Generator().manual_seed(11)
    per = 16
    lr, b1, b2, eps = R.f32(1e-3), R.f32(0.9), R.f32(0.999), R.f32(1e-8)
    scales, decays = [R.f32(s) for s in SCALES], [R.f32(w) for w in DECAYS]
    ps = [torch.randn(per, generator=gen, dtype=torch.float64).requires_grad_(True) for _ in SCALES]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([dict(params=[p], lr=lr * s, weight_decay=w) for p, s, w in zip(ps, scales, decays)], lr=lr, betas=(b1, b2), eps=eps,
              amsgrad=amsgrad)
    n = per * len(SCALES)
    grp = torch.arange(n) // per
    s_e, wd_e = torch.tensor(scales, dtype=torch.float64)[grp], torch.tensor(decays, dtype=torch.float64)[grp]
    p = torch.cat([q.detach() for q in ps]).clone()
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    vmax = torch.zeros(n, dtype=torch.float64) if amsgrad else None
    for t in range(1, 6):
        g = torch.randn(n, generator=gen, dtype=torch.float64)
        for q, gq in zip(ps, g.split(per)):
            q.grad = gq.clone()
        opt.step()
        hp = R.Hyper(lr, b1, b2, eps, 0.0, 1.0, t, 1.0 - b1 ** t, math.sqrt(1.0 - b2 ** t), 1)
        r = G.grouped_ref(p, m, v, g, hp, s_e, wd_e, decoupled, vmax)
        p, m, v, vmax = r["p"], r["m"], r["v"], r["vmax"]
        want = torch.cat([q.detach() for q in ps])
        assert float(((p - want).abs() / want.abs().clamp_min(1e-30)).max()) <= 1e-12, f"step {t}"


# ---------------------------------------------------------------------------------------------------------------
# schedule
# ---------------------------------------------------------------------------------------------------------------
LR0, W, T, RATIO = R.f32(3e-4), 5, 17, R.f32(0.1)


def _torch_lrs(make, steps):
    """get_last_lr() before the first and after each of `steps` scheduler steps."""
    opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=LR0)
    sch = make(opt)
    out = [sch.get_last_lr()[0]]
    for _ in range(steps):
        opt.step()
        sch.step()
        out.append(sch.get_last_lr()[0])
    return out


def _close(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


def test_sched_ref_phases_are_the_torch_schedulers():
    from torch.optim.lr_scheduler import CosineAnnealingLR, LinearLR
    warm = _torch_lrs(lambda o: LinearLR(o, start_factor=1.0 / W, end_factor=1.0, total_iters=W - 1), W + 1)
    for t in range(1, W + 3):                                   # step t is applied under the rate after t - 1 scheduler steps
        assert _close(G.sched_ref(t, LR0, 0.1, [], W, 0, 0, 0.0), warm[t - 1]), t
    lin = _torch_lrs(lambda o: LinearLR(o, start_factor=1.0, end_factor=RATIO, total_iters=T - W), T - W + 5)
    cos = _torch_lrs(lambda o: CosineAnnealingLR(o, T_max=T - W, eta_min=RATIO * LR0), T - W)
    for t in range(W, T + 6):                                   # the decay's clock starts at t = W: x = (t - W) / (T - W)
        assert _close(G.sched_ref(t, LR0, 0.1, [], W, 1, T, RATIO), lin[t - W]), t
        if t <= T:                                              # past T CosineAnnealingLR climbs again, the schedule stays
            assert _close(G.sched_ref(t, LR0, 0.1, [], W, 2, T, RATIO), cos[t - W]), t
    assert all(G.sched_ref(t, LR0, 0.1, [], W, 2, T, RATIO) == G.sched_ref(T, LR0, 0.1, [], W, 2, T, RATIO) for t in (T + 1, T + 50))
    # warm-up and decay multiply, and the milestones' gamma^k on top
    assert _close(G.sched_ref(3, LR0, 0.1, [2], W, 1, T, RATIO), LR0 * R.f32(0.1) * (3 / W))
    assert G.sched_ref(7, LR0, 0.1, [2, 4], 0, 0, 0, 0.0) == R.step_state_ref(7, LR0, 0.1, [2, 4], 0.9, 0.999)[0]


def test_sched_judge_accepts_f32_rounding_and_rejects_a_late_warmup():
    for kind in (0, 1, 2):
        for t in (1, W - 1, W, W + 1, T - 1, T, T + 5):
            ref = G.sched_ref(t, LR0, 0.1, [], W, kind, T, RATIO)
            assert G.sched_ratio(F(ref), ref, LR0) <= 1.0
    for t in range(1, W):                                       # warm-up (t - 1) / W: one step late
        ref = G.sched_ref(t, LR0, 0.1, [], W, 0, 0, 0.0)
        assert G.sched_ratio(F(LR0 * (t - 1) / W), ref, LR0) > 1.0
    assert G.sched_ratio(0.0, 0.0, LR0) == 0.0 and G.sched_ratio(F(LR0 * 2.0 ** -40), 0.0, LR0) > 1.0


def test_engine_host_mirror_is_sched_ref():
    from kvq.engine import lr_schedule_factor
    for kind, name in ((0, "none"), (1, "linear"), (2, "cosine")):
        for t in range(1, T + 6):
            want = G.sched_ref(t, LR0, 0.1, [], W, kind, T if kind else 0, RATIO)
            assert _close(LR0 * lr_schedule_factor(t, W, name, T if kind else 0, RATIO), want), (name, t)
