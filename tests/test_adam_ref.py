"""CPU self-check of tests/_adam_ref.py: the reference is torch.optim.Adam, every judge accepts an op-by-op numpy float32
restatement of adam_update4 / step_state_advance_sched_kernel (csrc/kvq_adam.hip) on the full input generator and rejects each planted
mistake on the same inputs, and the generator stays clear of the denormals.  Measured figures: profiles/adam_parity.md."""
import math

import numpy as np
import pytest
import torch

import _adam_ref as R

CASES = R.covering_cases()
ALL3 = R.ALL3
HOST_BC_CASES = R.BC_CASES       # the host entry's bias correction before it was computed in double: where the defect was measured


def _bc_f32(beta, t):
    """1.0f - powf(beta, t) in f32."""
    return np.float32(1.0) - np.power(np.float32(beta), np.float32(t), dtype=np.float32)


def _bc_pair(c, t):
    hp = R.hyper(R.LR, c.betas[0], c.betas[1], R.ADAM_EPS, c.wd, c.grad_scale, t)
    return np.float32(hp.bc1), np.float32(hp.bc2s)


def restate(x, c, coef=None, mistake=None):
    """adam_update4 in numpy float32, one rounding per operation, in the kernel's order; `mistake` plants one deviation.
    Returns dict(p, m, v, vmax) of torch f32 tensors."""
    F = np.float32
    lr, b1, b2, eps, wd, gs = (F(z) for z in (R.LR, c.betas[0], c.betas[1], R.ADAM_EPS, c.wd, c.grad_scale))
    if coef is not None:
        gs = gs * F(coef)                                              # adam_kernel: grad_scale *= guard->coef
    bc1, bc2s = _bc_pair(c, c.t)                                       # one f32 rounding of the f64 value
    if mistake == "bias corrections of step t-1":
        bc1, bc2s = _bc_pair(c, c.t - 1)
    if mistake == "f32 1.0f - powf(beta, t) bias corrections":
        bc1, bc2s = _bc_f32(c.betas[0], c.t), np.sqrt(_bc_f32(c.betas[1], c.t))
    p, m, v = (x[k].numpy().copy() for k in ("p", "m", "v"))
    g = x["g"].float().numpy()
    assert p.dtype == m.dtype == v.dtype == g.dtype == np.float32
    one = F(1.0)
    with np.errstate(all="ignore"):
        gv = g * gs
        if mistake == "grad_scale applied after the weight-decay term":
            gv = (g + p * wd) * gs
        elif mistake != "decoupled (AdamW) weight decay":
            gv = gv + p * wd
        m1 = m * b1 + gv * (one - b1)
        v1 = v * b2 + (gv * gv) * (one - b2)
        d, vm1 = v1, None
        if c.amsgrad:
            vmax = x["vmax"].numpy()
            vm1 = np.maximum(vmax, v1)
            d = vm1
            if mistake == "den from v' when amsgrad is on":
                d = v1
            if mistake == "vmax follows v' down when v' < vmax":
                vm1 = v1.copy()
            if mistake == "vmax not stored when v' > vmax":
                vm1 = vmax.copy()
        if mistake == "eps inside the square root":
            den = np.sqrt(d + eps) / bc2s
        elif mistake == "eps added before the division by bc2s":
            den = (np.sqrt(d) + eps) / bc2s
        elif mistake == "bc2 used without the square root":
            den = np.sqrt(d) / (bc2s * bc2s) + eps
        else:
            den = np.sqrt(d) / bc2s + eps
        step = lr / bc1
        if mistake == "decoupled (AdamW) weight decay":
            p = p - (lr * wd) * p
        p1 = p - step * (m1 / den)
    assert p1.dtype == m1.dtype == v1.dtype == np.float32
    t = torch.from_numpy
    return dict(p=t(p1), m=t(m1), v=t(v1), vmax=t(vm1) if vm1 is not None else None)


def judge_all(out, x, c, coef=None):
    """The worst ratio of every judge for one launch: dict(m, v[, vmax], p); a vmax that is not the exact maximum counts as inf."""
    return {k: float(r.max()) for k, r in R.launch_ratios(out, x, R.case_hyper(c, coef)).items()}


def _differs(c):
    return _bc_pair(c, c.t) != _bc_pair(c, c.t - 1)


# mistake -> the launches in which it changes the result at all
MISTAKES = {
    "eps inside the square root": lambda c: True,
    "eps added before the division by bc2s": lambda c: _bc_pair(c, c.t)[1] != 1,
    "decoupled (AdamW) weight decay": lambda c: c.wd != 0,
    "bc2 used without the square root": lambda c: _bc_pair(c, c.t)[1] != 1,
    "bias corrections of step t-1": lambda c: c.t >= 2 and _differs(c),
    "den from v' when amsgrad is on": lambda c: c.amsgrad,
    "vmax follows v' down when v' < vmax": lambda c: c.amsgrad,
    "vmax not stored when v' > vmax": lambda c: c.amsgrad,
    "grad_scale applied after the weight-decay term": lambda c: c.wd != 0 and c.grad_scale != 1,
}


def test_covering_set():
    R.assert_covering(CASES)
    assert 24 <= len(CASES) <= 48
    for name, applies in MISTAKES.items():
        assert any(applies(c) and c.n == ALL3 for c in CASES), f"no launch of all three paths in which '{name}' shows"


@pytest.mark.parametrize("amsgrad", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_reference_is_torch_adam(amsgrad, wd):
    """adam_ref iterated over 20 steps against torch.optim.Adam on float64 CPU tensors, the f32-rounded scalars given to torch as
    Python floats: 1e-12 relative.  This anchors the reference to torch's semantics, nothing else."""
    gen = torch.Generator().manual_seed(7)
    n = 64
    lr, b1, b2, eps = R.f32(1e-3), R.f32(0.9), R.f32(0.999), R.f32(1e-8)
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    tp = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=R.f32(wd), amsgrad=amsgrad)
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    vmax = torch.zeros(n, dtype=torch.float64) if amsgrad else None
    for t in range(1, 21):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * 10.0 ** float(torch.randint(-6, 2, (1,), generator=gen))
        tp.grad = g.clone()
        opt.step()
        out = R.adam_ref(p, m, v, g, R.hyper(lr, b1, b2, eps, wd, 1.0, t), vmax)
        p, m, v, vmax = out["p"], out["m"], out["v"], out["vmax"]
        st = opt.state[tp]
        torch.testing.assert_close(p, tp.detach(), rtol=1e-12, atol=0)
        torch.testing.assert_close(m, st["exp_avg"], rtol=1e-12, atol=0)
        torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-12, atol=0)
        if amsgrad:
            torch.testing.assert_close(vmax, st["max_exp_avg_sq"], rtol=1e-12, atol=0)


def test_reference_scales_the_gradient_before_the_decay_term():
    """grad_scale is torch's gradient multiplied beforehand: adam_ref(g, gs) == adam_ref(g * gs, 1) with wd on."""
    x = R.adam_inputs(64, 1)
    a = R.adam_ref(x["p"], x["m"], x["v"], x["g"], R.hyper(1e-3, 0.9, 0.999, 1e-8, 0.01, 0.25, 3))
    b = R.adam_ref(x["p"], x["m"], x["v"], x["g"].double() * 0.25, R.hyper(1e-3, 0.9, 0.999, 1e-8, 0.01, 1.0, 3))
    assert all(torch.equal(a[k], b[k]) for k in ("p", "m", "v"))


def test_judges_accept_the_f32_restatement():
    worst = {}
    for c in CASES + HOST_BC_CASES:
        x = R.case_inputs(c)
        for coef in (None, 1.0, 0.37):
            res = judge_all(restate(x, c, coef), x, c, coef)
            for k, r in res.items():
                key = (k, "guarded" if coef is not None else "plain")
                if r > worst.get(key, (-1.0, None))[0]:
                    worst[key] = (r, c)
    for (k, kind), (r, c) in sorted(worst.items()):
        print(f"FIGURE f32 restatement, {kind} {k}': worst ratio {r:.4f} (n = {c.n}, {c.gdtype}, betas {c.betas}, t = {c.t}, "
              f"wd = {c.wd}, grad_scale = {c.grad_scale:.4g})")
    assert set(k for k, _ in worst) == {"m", "v", "vmax", "p"}
    assert all(r <= 1.0 for r, _ in worst.values()), worst


@pytest.mark.parametrize("mistake", sorted(MISTAKES))
def test_judges_reject(mistake):
    """Rejected (some ratio > 1) in every launch of all three paths in which the mistake changes anything; the small launches
    (a handful of elements, where e.g. no sqrt(v) may lie near eps) are counted and at least one launch overall must reject."""
    applies = MISTAKES[mistake]
    seen = rejected = 0
    for c in CASES:
        if not applies(c):
            continue
        x = R.case_inputs(c)
        res = judge_all(restate(x, c, None, mistake), x, c)
        seen += 1
        rejected += max(res.values()) > 1.0
        if c.n == ALL3:
            assert max(res.values()) > 1.0, f"'{mistake}' was accepted at {c}: {res}"
    print(f"FIGURE '{mistake}': rejected in {rejected} of the {seen} launches in which it applies")
    assert seen and rejected


@pytest.mark.parametrize("c", HOST_BC_CASES, ids=lambda c: f"beta2={c.betas[1]}")
def test_p_judge_rejects_the_f32_bias_correction(c):
    """bc2s = sqrtf(1.0f - powf(beta2, 2)) is off by 3.3e-6 (beta2 = 0.999) and 2.5e-5 (0.9999) relative: the p' judge sees it,
    the moments (which do not use it) stay accepted."""
    mistake = "f32 1.0f - powf(beta, t) bias corrections"
    hp = R.case_hyper(c)
    rel = abs(float(np.sqrt(_bc_f32(c.betas[1], 2))) - hp.bc2s) / hp.bc2s
    x = R.case_inputs(c)
    res = judge_all(restate(x, c, None, mistake), x, c)
    print(f"FIGURE f32 bias correction at beta2 = {c.betas[1]}, t = 2: bc2s off by {rel:.3g} relative ({rel / R.EPS:.1f} EPS), p' ratio {res['p']:.2f}")
    assert rel > 20 * R.EPS
    assert res["p"] > 1.0 and res["m"] <= 1.0 and res["v"] <= 1.0
    assert judge_all(restate(x, c), x, c)["p"] <= 1.0


def test_generator_stays_clear_of_the_denormals():
    """Non-vacuity of the counted bounds: every non-zero intermediate of the f64 reference is at least 2^-100 (and finite in f32),
    so no f32 operation of a correct kernel underflows; the inputs hold what the docstring of adam_inputs promises."""
    lo, hi = math.inf, 0.0
    for c in CASES + HOST_BC_CASES:
        x = R.case_inputs(c)
        for coef in (None, 1.0, 0.37):
            ref = R.adam_ref(x["p"], x["m"], x["v"], x["g"], R.case_hyper(c, coef), x["vmax"], intermediates=True)
            for name, val in ref["all"].items():
                a = val.abs()
                nz = a[a != 0]
                assert torch.all(torch.isfinite(a)), name
                if nz.numel():
                    lo, hi = min(lo, float(nz.min())), max(hi, float(nz.max()))
                    assert float(nz.min()) >= R.TINY, f"{name} reaches {float(nz.min()):.3g} in {c}"
                    assert float(nz.max()) < 2.0 ** 100, name
    print(f"FIGURE intermediates of the reference lie in [{lo:.3g}, {hi:.3g}]; 2^-100 = {R.TINY:.3g}")
    big = R.adam_inputs(1 << 16, 5, torch.bfloat16, True)
    g = big["g"].float()
    assert bool((g == 0).any()) and float(g[g != 0].abs().min()) < 1e-11 and float(g.abs().max()) > 50
    assert bool((big["p"] == 0).any()) and bool((big["vmax"] > big["v"]).any()) and bool((big["vmax"] < big["v"]).any())
    root = big["v"].double().sqrt()
    assert float(root.min()) < 1e-3 * R.ADAM_EPS and float(root.max()) > 1e3 * R.ADAM_EPS
    ref = R.adam_ref(big["p"], big["m"], big["v"], big["g"], R.hyper(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 5), big["vmax"])
    assert bool((ref["v"] > big["vmax"].double()).any()) and bool((ref["v"] < big["vmax"].double()).any()), "both arms of the max"


# ---------------------------------------------------------------------------------------------------------------
# step state
# ---------------------------------------------------------------------------------------------------------------
def restate_step_state(t, lr0, gamma, milestones, beta1, beta2, mistake=None):
    """step_state_advance_sched_kernel without a schedule: f64 arithmetic on the f32 arguments, each field cast to f32 once."""
    k = sum(1 for ms in milestones if ((t - 1 > ms) if mistake == "milestone >" else (t - 1 >= ms)))
    lr = np.float64(np.float32(lr0))
    for _ in range(k):
        lr = lr * np.float64(np.float32(gamma))
    if mistake == "f32 powf":
        return float(np.float32(lr)), float(_bc_f32(beta1, t)), float(np.sqrt(_bc_f32(beta2, t)))
    b1, b2 = np.float64(np.float32(beta1)), np.float64(np.float32(beta2))
    return (float(np.float32(lr)), float(np.float32(1.0 - np.power(b1, np.float64(t)))),
            float(np.float32(np.sqrt(1.0 - np.power(b2, np.float64(t))))))


def test_step_state_judge():
    worst = 0.0
    for t in (1, 2, 10, 1000, 10 ** 6, 2 ** 32 + 5):
        for ms in ([], [t - 1], [t], [max(t - 2, 0)], [max(t - 2, 0), t - 1, t + 5], list(range(max(t - 4, 0), max(t - 4, 0) + 8))):
            for gamma in (0.1, 0.5):
                for b1, b2 in R.AXES["betas"]:
                    ref = R.step_state_ref(t, 1e-3, gamma, ms, b1, b2)
                    worst = max([worst] + R.step_state_ratios(restate_step_state(t, 1e-3, gamma, ms, b1, b2), ref))
                    if t - 1 in ms:
                        bad = R.step_state_ratios(restate_step_state(t, 1e-3, gamma, ms, b1, b2, "milestone >"), ref)
                        assert bad[0] > 1.0, "a milestone comparison with > instead of >= was accepted"
    print(f"FIGURE step-state restatement: worst ratio {worst:.4f}")
    assert worst <= 1.0
    assert R.step_state_ref(3, 1e-2, 0.1, [2, 4], 0.9, 0.999)[0] == R.f32(1e-2) * R.f32(0.1)
    assert R.step_state_ref(2, 1e-2, 0.1, [2, 4], 0.9, 0.999)[0] == R.f32(1e-2)
    for b2 in (0.999, 0.9999):
        bad = R.step_state_ratios(restate_step_state(2, 1e-3, 0.1, [], 0.9, b2, "f32 powf"), R.step_state_ref(2, 1e-3, 0.1, [], 0.9, b2))
        print(f"FIGURE f32 1.0f - powf at beta2 = {b2}, t = 2: step-state ratios (lr, bc1, bc2s) = {[round(r, 2) for r in bad]}")
        assert bad[2] > 1.0


def test_paths_and_patterns():
    assert R.paths_of(1) == {"scalar tail"} and R.paths_of(4) == {"odd 4-chunk"} and R.paths_of(8) == {"8-chunk"}
    assert R.paths_of(15) == R.paths_of(ALL3) == {"8-chunk", "odd 4-chunk", "scalar tail"}
    code = R.path_codes(23)
    assert code.tolist() == [0] * 16 + [1] * 4 + [2] * 3
    assert "e mod 8 = 4" in R.describe(20, 23) and "scalar tail" in R.describe(22, 23)
    n = R.ADAM_TRIP + 8 * 3 + 4 + 3
    code = R.path_codes(n)
    assert int((code == 3).sum()) == 24 and int(code[R.ADAM_TRIP - 1]) == 0 and int(code[R.ADAM_TRIP]) == 3
    assert code[-7:].tolist() == [1, 1, 1, 1, 2, 2, 2] and R.ADAM_TRIP == 67108864
    # the integer RNE of the shadow judge against torch's conversion, on the tie patterns and on random values
    pat = R.shadow_patterns()
    x = torch.cat([pat, torch.randn(4096) * 3])
    x = x[torch.isfinite(x.bfloat16().float()) | torch.isfinite(x)]
    assert torch.equal(R.bf16_rne_bits(x), R.bf16_bits(x.bfloat16()))
    one_tie_even = torch.tensor([0x3F808000], dtype=torch.int32).view(torch.float32)
    one_tie_odd = torch.tensor([0x3F818000], dtype=torch.int32).view(torch.float32)
    assert R.bf16_rne_bits(one_tie_even).item() == 0x3F80 and R.bf16_rne_bits(one_tie_odd).item() == 0x3F82
    top = torch.tensor([0x7F7F7FFF, 0x7F7F8000], dtype=torch.int32).view(torch.float32)
    assert R.bf16_rne_bits(top).tolist() == [0x7F7F, 0x7F80]
