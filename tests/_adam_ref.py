"""f64 references, input generator and judges for the Adam kernels and the step state (adam_kernel, step_state_advance_sched_kernel of
csrc/kvq_adam.hip; tests/test_adam_parity_gpu.py).  Everything here is plain torch on whatever device its inputs live on (the CPU,
or the GPU in f64 for the grid-stride cases); tests/test_adam_ref.py shows on the CPU that each judge accepts an op-by-op f32
restatement of the kernel and rejects planted mistakes.

Every judge returns a per-element ratio |kernel - reference| / bound; at most 1 passes.  The bounds count f32 roundings: the
library is built with -ffp-contract=off, so each f32 operation (+ - * / sqrt, correctly rounded) returns exact * (1 + d) with
|d| <= EPS = 2^-24, and k such factors stay within GAMMA(k) = k EPS / (1 - k EPS).  No constant here was fitted to a kernel's
output; each has its count beside it."""
import math
from collections import namedtuple

import numpy as np
import torch

EPS = 2.0 ** -24                 # unit roundoff of f32, round to nearest even
TINY = 2.0 ** -100               # the generator keeps every non-zero intermediate above this (far above the f32 denormals)
ADAM_BLOCK_CAP = 32768           # adam_launch: at most this many blocks of 256 threads, 8 elements per thread and loop trip
ADAM_TRIP = ADAM_BLOCK_CAP * 256 * 8


def GAMMA(k):
    return k * EPS / (1.0 - k * EPS)


def f32(x):
    """A Python float rounded to f32: what a `float` argument of the C ABI receives."""
    return float(np.float32(x))


Hyper = namedtuple("Hyper", "lr beta1 beta2 eps wd grad_scale t bc1 bc2s gs_roundings")


def hyper(lr, beta1, beta2, eps, wd, grad_scale, t, coef=None):
    """The scalars of one step as the kernel's arithmetic sees them: each rounded to f32, then f64.  bc1 = 1 - beta1^t and
    bc2s = sqrt(1 - beta2^t) in f64 from the rounded betas.  coef: the guarded entries multiply the guard's f32 coefficient into
    grad_scale IN f32 (one more rounding on the g * grad_scale term, counted in gs_roundings); here the product stays exact."""
    b1, b2 = f32(beta1), f32(beta2)
    gs = f32(grad_scale) * (f32(coef) if coef is not None else 1.0)
    t = int(t)
    return Hyper(f32(lr), b1, b2, f32(eps), f32(wd), gs, t, 1.0 - math.pow(b1, t), math.sqrt(1.0 - math.pow(b2, t)),
                 2 if coef is not None else 1)


def adam_ref(p, m, v, g, hp, vmax=None, intermediates=False):
    """One torch.optim.Adam step (coupled L2 weight decay, optional amsgrad) in f64 from the f32 pre-state and the f32 / bf16
    gradient.  Returns dict(p, m, v, vmax or None) and, with intermediates=True, every intermediate under "all"."""
    p, m, v, g = p.double(), m.double(), v.double(), g.double()
    gg = g * hp.grad_scale
    wp = hp.wd * p
    g1 = gg + wp
    m_a, m_b = hp.beta1 * m, (1.0 - hp.beta1) * g1
    m1 = m_a + m_b
    sq = g1 * g1
    v_a, v_b = hp.beta2 * v, (1.0 - hp.beta2) * sq
    v1 = v_a + v_b
    vm1 = torch.maximum(vmax.double(), v1) if vmax is not None else None
    root = torch.sqrt(vm1 if vmax is not None else v1)
    den = root / hp.bc2s + hp.eps
    q = m1 / den
    u = (hp.lr / hp.bc1) * q
    out = dict(p=p - u, m=m1, v=v1, vmax=vm1)
    if intermediates:
        out["all"] = dict(gg=gg, wp=wp, g1=g1, m_a=m_a, m_b=m_b, m1=m1, sq=sq, v_a=v_a, v_b=v_b, v1=v1, root=root, den=den, q=q, u=u,
                          p1=out["p"])
    return out


def update_ref(m1, den_src, hp):
    """The f64 update lr / bc1 * m' / (sqrt(den_src) / bc2s + eps) from STORED f32 moments (exact inputs)."""
    return (hp.lr / hp.bc1) * (m1.double() / (torch.sqrt(den_src.double()) / hp.bc2s + hp.eps))


# ---------------------------------------------------------------------------------------------------------------
# judges
# ---------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    """err / bound with 0 / 0 = 0 (an exact zero against a zero bound passes, anything else against a zero bound does not)."""
    return torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))


def moment_ratios(got_m, got_v, got_vmax, p, m, v, g, hp, vmax=None):
    """Ratios for m', v' (and vmax') against adam_ref of the identical f32 pre-state.  Roundings, per term of the result:

    g' = fl(fl(g * gs) + fl(p * wd)):  the g term carries r = 1 + gs_roundings (its product, [the guard's gs * coef,] the sum), the
         wd p term 2 (its product, the sum): |g'_f32 - g'| <= e := GAMMA(r) |g gs| + GAMMA(2) |wd p|.
    m' = fl(fl(m * b1) + fl(g' * fl(1 - b1))):  the m term 2 (product, sum); the g' terms 3 more (1 - b1, product, sum):
         bound_m = GAMMA(2) b1 |m| + (1 - b1) (GAMMA(r + 3) |g gs| + GAMMA(5) |wd p|)          r + 3 = 5, guarded 6
    v' = fl(fl(v * b2) + fl(fl(g' * g') * fl(1 - b2))):  the v term 2; with G = |g gs| + |wd p| >= |g'| the square of the rounded
         g' is off by at most e (2 G + e), and the square, 1 - b2, the product and the sum round 4 more times:
         bound_v = GAMMA(2) b2 v + (1 - b2) (e (2 G + e) (1 + GAMMA(4)) + GAMMA(4) G^2)          <= (2 r + 4) EPS (1 - b2) G^2 + ...
    vmax' = max(vmax, v'): |max(a, x) - max(a, y)| <= |x - y|, so bound_v again (max itself is exact: launch_ratios checks that).
    The bounds are relative to these magnitude sums, not to |m'|: the two terms of m' can cancel."""
    ref = adam_ref(p, m, v, g, hp, vmax)
    pd, md, vd, gd = p.double(), m.double(), v.double(), g.double()
    agg, awp = (gd * hp.grad_scale).abs(), (hp.wd * pd).abs()
    r = 1 + hp.gs_roundings
    e = GAMMA(r) * agg + GAMMA(2) * awp
    G = agg + awp
    bound_m = GAMMA(2) * hp.beta1 * md.abs() + (1.0 - hp.beta1) * (GAMMA(r + 3) * agg + GAMMA(5) * awp)
    bound_v = GAMMA(2) * hp.beta2 * vd + (1.0 - hp.beta2) * (e * (2 * G + e) * (1 + GAMMA(4)) + GAMMA(4) * G * G)
    out = dict(m=_ratio((got_m.double() - ref["m"]).abs(), bound_m), v=_ratio((got_v.double() - ref["v"]).abs(), bound_v))
    if vmax is not None:
        out["vmax"] = _ratio((got_vmax.double() - ref["vmax"]).abs(), bound_v)
    return out


def p_ratio(got_p, p, got_m, got_den_src, hp):
    """Ratio for p' against p - u_ref, u_ref = update_ref of the kernel's own STORED m' and v' (vmax' with amsgrad), so this bound
    does not inherit the moments'.  The kernel's u = fl(fl(lr / bc1_f32) * fl(m' / den)), den = fl(fl(fl(sqrt(d)) / bc2s_f32) + eps):
      den:  sqrt, the division and the f32 rounding of bc2s are 3 on sqrt(d) / bc2s, the sum of two positive terms 1 more    -> 4
      m' / den: its own rounding                                                                                             -> 5
      lr / bc1: the division and the f32 rounding of bc1                                                                      -> 2
      the product                                                                                                             -> 1
    |u - u_ref| <= GAMMA(8) |u_ref|; the final subtraction rounds once more, EPS |p - u| (half an ulp of the result):
      bound = GAMMA(8) |u_ref| + EPS (|p - u_ref| + GAMMA(8) |u_ref|)
    With p = 0 the stored value is -u at full resolution and the bound is 9 EPS |u_ref|."""
    u = update_ref(got_m, got_den_src, hp)
    want = p.double() - u
    du = GAMMA(8) * u.abs()
    bound = du + EPS * (want.abs() + du)
    return _ratio((got_p.double() - want).abs(), bound)


def launch_ratios(out, x, hp):
    """Every judge on one launch: out = dict(p, m, v, vmax) as stored (f32), x = the pre-state and gradient (adam_inputs), on one
    device.  dict(m, v[, vmax], p) of per-element ratios; a stored vmax' that is not the exact maximum gets inf."""
    ams = x["vmax"] is not None
    r = moment_ratios(out["m"], out["v"], out["vmax"], x["p"], x["m"], x["v"], x["g"], hp, x["vmax"])
    r["p"] = p_ratio(out["p"], x["p"], out["m"], out["vmax"] if ams else out["v"], hp)
    if ams:
        r["vmax"] = torch.where(out["vmax"] != torch.maximum(x["vmax"], out["v"]), torch.full_like(r["vmax"], math.inf), r["vmax"])
    return {k: torch.nan_to_num(v, nan=math.inf) for k, v in r.items()}


def step_state_ref(t, lr0, gamma, milestones, beta1, beta2):
    """(lr, bc1, bc2s) of step t (1-based) as include/kvq.h states them: lr0 gamma^k with k = #{milestones <= t - 1},
    1 - beta1^t, sqrt(1 - beta2^t); f64 from the f32-rounded arguments."""
    t = int(t)
    k = sum(1 for ms in milestones if int(ms) <= t - 1)
    b1, b2 = f32(beta1), f32(beta2)
    return f32(lr0) * f32(gamma) ** k, 1.0 - math.pow(b1, t), math.sqrt(1.0 - math.pow(b2, t))


STEP_STATE_BOUND = 2.0 ** -23    # each field is ONE f32 rounding of an f64 value (error of the f64 arithmetic: ~1e-15)


def step_state_ratios(got, ref):
    """|got - ref| / (2^-23 |ref|) for (lr, bc1, bc2s)."""
    return [abs(float(a) - b) / (STEP_STATE_BOUND * abs(b)) for a, b in zip(got, ref)]


# ---------------------------------------------------------------------------------------------------------------
# which part of adam_kernel handles an element
# ---------------------------------------------------------------------------------------------------------------
PATHS = ("8-chunk", "odd 4-chunk", "scalar tail", "loop trip >= 2")


def path_codes(n, device="cpu"):
    """int8 tensor [n]: index into PATHS of the code that updates each element (adam_kernel / adam_launch)."""
    n4 = n // 4
    n8 = n4 // 2
    blocks = max(1, min(((n4 + 1) // 2 + 255) // 256, ADAM_BLOCK_CAP))
    code = torch.zeros(n, dtype=torch.int8, device=device)
    first_trip = min(8 * n8, blocks * 256 * 8)
    code[first_trip:8 * n8] = 3
    code[8 * n8:4 * n4] = 1
    code[4 * n4:] = 2
    return code


def paths_of(n):
    return {PATHS[int(c)] for c in torch.unique(path_codes(n))}


def path_of(e, n):
    """PATHS entry of one element (path_codes without the tensor)."""
    n4 = n // 4
    n8 = n4 // 2
    blocks = max(1, min(((n4 + 1) // 2 + 255) // 256, ADAM_BLOCK_CAP))
    if e < 8 * n8:
        return PATHS[0] if e < blocks * 256 * 8 else PATHS[3]
    return PATHS[1] if e < 4 * n4 else PATHS[2]


def describe(e, n):
    """Where element e of an n-element launch went: for failure reports."""
    return f"element {e} of {n} (e mod 8 = {e % 8}, {path_of(e, n)})"


def worst(ratio, n, first=0):
    """(worst ratio, description of its element); `first`: index of ratio[0] when a slice is judged."""
    r = torch.nan_to_num(ratio.detach(), nan=float("inf"))
    i = int(r.argmax())
    return float(r[i]), describe(first + i, n)


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def adam_inputs(n, seed, gdtype=torch.float32, amsgrad=False, device="cpu"):
    """Adversarial but legal pre-state and gradient of n elements:
      g     sign * 10^U(-12, 2) with one element in eight an exact zero, rounded to gdtype;
      v     a^2 with a = 10^U(-12, 2) (so sqrt(v) runs from far below eps = 1e-8 to far above), m = a * U(-1, 1) without zeros;
      vmax  v * U(0.5, 2): both arms of the max are taken;
      p     one third exact zeros (the stored p' is then the update at full f32 resolution), one third ~ 1e-3, one third ~ 1."""
    gen = torch.Generator(device=device).manual_seed(int(seed))
    rnd = lambda: torch.rand(n, generator=gen, device=device, dtype=torch.float64)
    sign = lambda: torch.where(rnd() < 0.5, -1.0, 1.0)
    g = sign() * 10.0 ** (rnd() * 14 - 12)
    g = torch.where(rnd() < 0.125, torch.zeros_like(g), g).float().to(gdtype)
    a = 10.0 ** (rnd() * 14 - 12)
    v = (a * a).float()
    m = (a * sign() * (0.05 + 0.95 * rnd())).float()
    vmax = (v.double() * (0.5 + 1.5 * rnd())).float() if amsgrad else None
    kind = rnd()
    mag = torch.where(kind < 2 / 3, 1e-3 * (1 + rnd()), 0.5 + rnd())
    p = torch.where(kind < 1 / 3, torch.zeros_like(mag), sign() * mag).float()
    return dict(p=p, m=m, v=v, vmax=vmax, g=g)


NS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 23, 2048 + 4 + 3)
AXES = dict(gdtype=(torch.float32, torch.bfloat16), amsgrad=(False, True), wd=(0.0, 0.01), grad_scale=(1.0, 1.0 / 3.0, 1024.0),
            betas=((0.9, 0.999), (0.5, 0.9999), (0.0, 0.98)), t=(1, 2, 5, 100, 1000, 10 ** 6))
Case = namedtuple("Case", "n gdtype amsgrad wd grad_scale betas t seed")
LR, ADAM_EPS = 1e-3, 1e-8


def covering_cases():
    """A few dozen launches instead of the Cartesian product: every n once with the other axes cycling at different strides,
    then 18 launches that alternate the two sizes holding all three of 8-chunk, odd 4-chunk and scalar tail (15 and 2055), in
    which every value of every axis occurs.  assert_covering states the property and is asserted by both test files."""
    ax = AXES
    pick = lambda i: dict(gdtype=ax["gdtype"][(i + i // 6) % 2], amsgrad=ax["amsgrad"][(i // 2) % 2], wd=ax["wd"][(i // 3) % 2],
                          grad_scale=ax["grad_scale"][(i + i // 3) % 3], betas=ax["betas"][(i // 2) % 3], t=ax["t"][i % 6])
    cases = [Case(n=n, seed=100 + i, **pick(i)) for i, n in enumerate(NS)]
    cases += [Case(n=(15, 2048 + 4 + 3)[i % 2], seed=200 + i, **pick(i + 1)) for i in range(18)]
    return cases


def assert_covering(cases):
    """Every value of every axis meets every code path (8-chunk, odd 4-chunk, scalar tail), and every n of NS occurs."""
    assert {c.n for c in cases} >= set(NS)
    for axis, values in AXES.items():
        for val in values:
            met = set()
            for c in cases:
                if getattr(c, axis) == val:
                    met |= paths_of(c.n)
            assert met >= {"8-chunk", "odd 4-chunk", "scalar tail"}, f"{axis} = {val} meets only {sorted(met)}"


ALL3 = 2048 + 4 + 3
# (beta2, t) = (0.999, 2) and (0.9999, 2): where a bias correction computed as 1.0f - powf(beta2, t) in f32 is off by 56 and 419 EPS
BC_CASES = [Case(n=ALL3, gdtype=torch.float32, amsgrad=False, wd=0.0, grad_scale=1.0, betas=b, t=2, seed=300 + i)
            for i, b in enumerate(((0.9, 0.999), (0.5, 0.9999)))]


def case_hyper(c, coef=None):
    return hyper(LR, c.betas[0], c.betas[1], ADAM_EPS, c.wd, c.grad_scale, c.t, coef)


def case_inputs(c, device="cpu"):
    return adam_inputs(c.n, c.seed, c.gdtype, c.amsgrad, device)


# ---------------------------------------------------------------------------------------------------------------
# bf16 rounding by integer arithmetic (the shadow)
# ---------------------------------------------------------------------------------------------------------------
def bf16_rne_bits(x):
    """int32 tensor of the bf16 bit patterns (0 .. 65535) of the RNE rounding of finite f32 x, from the f32 bits alone."""
    b = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).to(torch.int32)


def bf16_bits(x):
    """int32 tensor of the bit patterns of a bf16 tensor."""
    return x.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def shadow_patterns():
    """f32 values (as a tensor) on which RNE to bf16 is decided by the last bits: exact ties on even and odd bf16 neighbours, one
    f32 ulp above and below the tie, +-0, the largest finite f32 that still rounds to the bf16 maximum (and the tie above it, which
    rounds to infinity), and values across a power of two.  Both signs of each."""
    bits = []
    for hi in (0x3F80, 0x3F81, 0x3FFE, 0x3FFF, 0x0080, 0x4B7F, 0x3A83):          # even and odd bf16 neighbours, several exponents
        bits += [(hi << 16) | 0x8000, (hi << 16) | 0x8001, (hi << 16) | 0x7FFF, hi << 16]
    bits += [0x00000000, 0x7F7F7FFF, 0x7F7F8000, 0x7F7F0000]
    bits += [0x3F7FFFFF, 0x3F7F8000, 0x3F7F7FFF, 0x3F800000, 0x3F800001]            # across 1.0
    bits += [b | 0x80000000 for b in bits]
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())
