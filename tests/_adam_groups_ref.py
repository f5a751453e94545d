"""f64 reference and judges for the grouped / decoupled Adam update and the learning-rate schedule (adam_group_kernel,
step_state_advance_sched_kernel of csrc/kvq_adam.hip; include/kvq.h "parameter groups").  Built on tests/_adam_ref.py: the same input
generator, the same convention (every judge returns |kernel - reference| / bound per element, at most 1 passes) and the same kind
of bound -- counted f32 roundings, each count beside its term, no constant fitted to a kernel's output.
tests/test_adam_groups_ref.py shows on the CPU that the judges accept an op-by-op f32 restatement of the contract and reject
planted mistakes.

Per element of group j (lr, bc1, bc2s from the step state, c = grad_scale [* coef]):  lr_j = fl(lr * s_j);
  coupled    adam_update4's statements with wd_j for wd and lr_j for lr;
  decoupled  p0 = fl(p * fl(1 - fl(lr_j * wd_j))), the moments from g * c alone, p' = fl(p0 - u)."""
import math

import torch

from _adam_ref import EPS, GAMMA, STEP_STATE_BOUND, _ratio, adam_ref, f32, moment_ratios, update_ref

__all__ = ["element_groups", "element_tables", "grouped_ref", "grouped_ratios", "sched_ref", "sched_ratio", "SCHED_ABS"]


def element_groups(blocks, first_element, n):
    """Group id of each of the n elements of a launch that starts at `first_element` of the flat buffer: blocks[(first + e) >> 4]."""
    e = torch.arange(n, dtype=torch.int64, device=blocks.device) + int(first_element)
    return blocks.to(torch.int64)[e >> 4]


def element_tables(groups, scale, wd):
    """Per-element (s, wd) as f64 tensors from the f32 tables the kernel reads (exact in f64)."""
    s = torch.as_tensor(scale, dtype=torch.float32).double().to(groups.device)
    w = torch.as_tensor(wd, dtype=torch.float32).double().to(groups.device)
    return s[groups], w[groups]


def grouped_ref(p, m, v, g, hp, s_e, wd_e, decoupled, vmax=None):
    """One step of torch.optim.Adam (decoupled: torch.optim.AdamW) with per-element lr = hp.lr * s_e and weight decay wd_e, in f64 from
    the f32 pre-state.  dict(p, m, v, vmax or None).  hp: _adam_ref.hyper (its wd is not read)."""
    pd = p.double()
    lr_e = hp.lr * s_e
    if decoupled:
        p0 = pd * (1.0 - lr_e * wd_e)
        r = adam_ref(p, m, v, g, hp._replace(wd=0.0), vmax, intermediates=True)
    else:
        p0 = pd
        r = adam_ref(p, m, v, g, hp._replace(wd=wd_e), vmax, intermediates=True)
    u = (lr_e / hp.bc1) * r["all"]["q"]
    return dict(p=p0 - u, m=r["m"], v=r["v"], vmax=r["vmax"])


def grouped_p_ratio(got_p, p, got_m, got_den_src, hp, s_e, wd_e, decoupled):
    """Ratio for p' against p0 - u_ref, u_ref from the kernel's own STORED moments (as _adam_ref.p_ratio: the bound does not inherit
    the moments').  Roundings:
      u    = fl(fl(lr_j / bc1_f32) * fl(m' / den)): _adam_ref.p_ratio counts 8; lr_j = fl(lr * s_j) is one more            -> 9
      p0   (decoupled) = fl(p * fl(1 - fl(lr_j * wd_j))) = p (keep - x theta_2)(1 + theta'_2) with x = lr_j wd_j, keep = 1 - x: the keep
           term passes 2 roundings (the subtraction, the product with p), the x term 4 (lr_j, lr_j * wd_j, the subtraction, the
           product):  |p0_f32 - p0| <= |p| (GAMMA(2) |keep| + GAMMA(4) x);  coupled: p0 = p, exact
      p'   = fl(p0 - u): EPS |p0 - u| once more (half an ulp of the result)."""
    pd = p.double()
    lr_e = hp.lr * s_e
    u = update_ref(got_m, got_den_src, hp._replace(lr=1.0)) * lr_e
    if decoupled:
        x = lr_e * wd_e
        keep = 1.0 - x
        p0, dp0 = pd * keep, pd.abs() * (GAMMA(2) * keep.abs() + GAMMA(4) * x)
    else:
        p0, dp0 = pd, torch.zeros_like(pd)
    want = p0 - u
    du = GAMMA(9) * u.abs()
    bound = dp0 + du + EPS * (want.abs() + dp0 + du)
    return _ratio((got_p.double() - want).abs(), bound)


def grouped_ratios(out, x, hp, s_e, wd_e, decoupled):
    """Every judge on one launch (as _adam_ref.launch_ratios): out = dict(p, m, v, vmax) as stored, x = adam_inputs' pre-state.
    The moments are judged by _adam_ref.moment_ratios with the element's own wd (coupled) or none (decoupled: g' = g * c, the
    bound's wd p terms vanish); a stored vmax' that is not the exact maximum gets inf."""
    ams = x["vmax"] is not None
    wd_m = torch.zeros_like(wd_e) if decoupled else wd_e
    r = moment_ratios(out["m"], out["v"], out["vmax"], x["p"], x["m"], x["v"], x["g"], hp._replace(wd=wd_m), x["vmax"])
    r["p"] = grouped_p_ratio(out["p"], x["p"], out["m"], out["vmax"] if ams else out["v"], hp, s_e, wd_e, decoupled)
    if ams:
        r["vmax"] = torch.where(out["vmax"] != torch.maximum(x["vmax"], out["v"]), torch.full_like(r["vmax"], math.inf), r["vmax"])
    return {k: torch.nan_to_num(val, nan=math.inf) for k, val in r.items()}


# ---------------------------------------------------------------------------------------------------------------
# learning-rate schedule
# ---------------------------------------------------------------------------------------------------------------
def sched_ref(t, lr0, gamma, milestones, warmup_steps, decay_kind, total_steps, min_ratio):
    """lr of the 1-based step t as include/kvq.h states kvq_step_state_advance_sched, in f64 from the f32-rounded arguments:
    lr0 gamma^k warm dec;  decay_kind 0 none, 1 linear, 2 cosine."""
    t, W, T = int(t), int(warmup_steps), int(total_steps)
    k = sum(1 for ms in milestones if int(ms) <= t - 1)
    r = f32(min_ratio)
    warm = t / W if W > 0 and t < W else 1.0
    dec = 1.0
    if decay_kind != 0:
        x = min(max((t - W) / (T - W), 0.0), 1.0)
        dec = 1.0 - (1.0 - r) * x if decay_kind == 1 else r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * x))
    return f32(lr0) * f32(gamma) ** k * warm * dec


# Where the decay reaches exactly 0 (min_ratio 0 at t >= T) a relative bound has nothing to hold on to, while a device cos(pi) may be
# one f64 ulp away from -1, leaving 1 + cos(pi) = 2^-53 instead of 0: there the f64 arithmetic is allowed a few roundings at 2^-53
# on values of at most lr0 (warm, dec <= 1), 2^-50 lr0 in all.
SCHED_ABS = 2.0 ** -50


def sched_ratio(got, ref, lr0):
    """|got - ref| / (2^-23 |ref|): one f32 rounding of the f64 value (_adam_ref.STEP_STATE_BOUND); for ref = 0, |got| / (2^-50 lr0)."""
    if ref == 0.0:
        return abs(float(got)) / (SCHED_ABS * abs(f32(lr0)))
    return abs(float(got) - ref) / (STEP_STATE_BOUND * abs(ref))
