"""The gradient guard kernels (csrc/kvq_gradnorm.hip, include/kvq.h "gradient guard"): the deterministic sum of squares, the guard
state kvq_grad_guard_finalize derives from it (norm, torch.nn.utils.clip_grad_norm_'s coefficient, the skip of a non-finite
gradient), and the Adam kernels behind a guard."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
EXACT_N = [1, 2, 3, 4, 7, 8, 9, 23, 4096 * 3, 2 ** 20 + 5]


def _partials(g, P=None):
    from kvq import nnops
    part = torch.full((P or nnops.grad_sumsq_partials(),), float("nan"), dtype=torch.float64, device="cuda")    # every slot must be written
    nnops.grad_sumsq_partial(g, part)
    return part


def _integers(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (n,), generator=g).to(dtype).cuda()


@pytest.mark.parametrize("dtype", DTYPES)
def test_sum_of_squares_of_small_integers_is_exact(dtype):
    """Integers in [-3, 3]: every intermediate of any correct accumulation order is an integer below 2^24, so the f64 sum of the
    partials IS (g.double() ** 2).sum().  Two calls give the same partials bit for bit."""
    from kvq import nnops
    assert nnops.grad_sumsq_partials() == 2048
    for n in EXACT_N:
        g = _integers(n, dtype, n)
        a, b = _partials(g), _partials(g)
        assert a.numel() == nnops.grad_sumsq_partials()
        want = (g.double() ** 2).sum().item()
        assert a.sum().item() == want, (n, a.sum().item(), want)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)), n


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_view_16_elements_into_a_buffer_gives_the_sum_of_the_view_only(dtype):
    buf = _integers(16 + 4096 * 3 + 5 + 16, dtype, 77)
    buf[:16] = 3
    buf[-16:] = 3
    view = buf[16:-16]
    assert _partials(view).sum().item() == (view.double() ** 2).sum().item()
    view = buf[16:16 + 23]
    assert _partials(view).sum().item() == (view.double() ** 2).sum().item()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [4096 * 3, 2 ** 20 + 5])
def test_sum_of_squares_of_random_values(dtype, n):
    """randn * 1e-3.  The kernel adds the 8 squares of a 16-byte chunk in f32 and everything above in f64 (not f64 throughout): the
    bound is 1e-6 relative to the f64 sum."""
    g = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 1e-3).to(dtype).cuda()
    got, want = _partials(g).sum().item(), (g.double() ** 2).sum().item()
    print(f"sumsq {dtype} n={n}: relative error {abs(got - want) / want:.3g}")
    assert abs(got - want) <= 1e-6 * want


def _finalize(g, max_norm, guard=None, pieces=1):
    from kvq import nnops
    P = nnops.grad_sumsq_partials()
    guard = nnops.new_grad_guard("cuda") if guard is None else guard
    part = torch.empty(pieces * P, dtype=torch.float64, device="cuda")
    cuts = [g.numel() * i // pieces // 16 * 16 for i in range(pieces)] + [g.numel()]
    for i in range(pieces):
        nnops.grad_sumsq_partial(g[cuts[i]:cuts[i + 1]], part[i * P:(i + 1) * P])
    nnops.grad_guard_finalize(part, max_norm, guard)
    return guard, nnops.read_grad_guard(guard)


@pytest.mark.parametrize("dtype", DTYPES)
def test_finalize_gives_norm_and_the_coefficient_of_clip_grad_norm(dtype):
    n = 4096 * 3 + 23
    g = (torch.randn(n, generator=torch.Generator().manual_seed(5)) * 1e-2).to(dtype).cuda()
    norm64 = math.sqrt((g.double() ** 2).sum().item())
    for max_norm in (0.37 * norm64, 2.5 * norm64, float("inf")):
        _, st = _finalize(g, max_norm, pieces=3)
        want_norm = torch.tensor(norm64, dtype=torch.float64).float().item()
        want_coef = torch.tensor(min(1.0, max_norm / (norm64 + 1e-6)), dtype=torch.float64).float().item()
        print(f"finalize {dtype} max_norm={max_norm:.4g}: norm {st['norm']!r} want {want_norm!r}, coef {st['coef']!r} want {want_coef!r}")
        assert abs(st["norm"] - want_norm) <= 5e-7 * want_norm
        assert abs(st["coef"] - want_coef) <= 5e-7 * want_coef
        assert st["skip"] == 0 and st["skipped"] == 0
        assert abs(st["sumsq"] - norm64 ** 2) <= 1e-6 * norm64 ** 2
        if max_norm > norm64:
            assert st["coef"] == 1.0
        # torch.nn.utils.clip_grad_norm_ on f64 copies of the gradient split into three tensors: what it multiplies the gradients by
        ps = [torch.nn.Parameter(torch.zeros(c.numel(), dtype=torch.float64)) for c in g.cpu().double().chunk(3)]
        for p, c in zip(ps, g.cpu().double().chunk(3)):
            p.grad = c.clone()
        total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        assert abs(total.item() - norm64) <= 1e-12 * norm64
        big = int(g.double().abs().argmax())                           # read it off the element with the largest gradient
        coef_torch = torch.cat([p.grad for p in ps])[big].item() / g.double()[big].item()
        assert abs(st["coef"] - coef_torch) <= 5e-7 * coef_torch, (st["coef"], coef_torch)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_non_finite_gradient_sets_skip(dtype):
    from kvq import nnops
    n = 4096 * 3 + 5
    base = (torch.randn(n, generator=torch.Generator().manual_seed(9)) * 1e-2).to(dtype).cuda()
    guard = nnops.new_grad_guard("cuda")
    calls = 0
    for bad in (float("inf"), float("-inf"), float("nan")):
        for pos in (0, n // 2, n - 1):
            g = base.clone()
            g[pos] = bad
            _, st = _finalize(g, 1.0, guard)
            calls += 1
            assert st["skip"] == 1 and st["coef"] == 0.0 and st["skipped"] == calls, (bad, pos, st)
            assert not math.isfinite(st["norm"]) and not math.isfinite(st["sumsq"])
    _, st = _finalize(base, 1.0, guard)                              # a finite gradient behind them: the flag is cleared, the count stays
    assert st["skip"] == 0 and 0.0 < st["coef"] <= 1.0 and st["skipped"] == calls and math.isfinite(st["norm"])


def test_a_finite_bf16_gradient_whose_square_overflows_sets_skip():
    from kvq import nnops
    g = torch.zeros(4096 * 3, dtype=torch.bfloat16, device="cuda")
    g[1234] = 1e20                                                   # finite in bf16, 1e40 is not an f32
    assert bool(torch.isfinite(g).all())
    guard = nnops.new_grad_guard("cuda")
    _, st = _finalize(g, float("inf"), guard)
    assert st["skip"] == 1 and st["coef"] == 0.0 and st["skipped"] == 1
    g[1234] = 1.0
    _, st = _finalize(g, float("inf"), guard)
    assert st["skip"] == 0 and st["coef"] == 1.0 and st["norm"] == 1.0 and st["skipped"] == 1


def _guard_with(coef=1.0, skip=0):
    """A guard state as kvq_grad_guard_finalize leaves it, written from the host."""
    from kvq import nnops
    guard = nnops.new_grad_guard("cuda")
    guard[1:2].view(torch.float32)[1] = coef
    guard[2] = skip
    return guard


def _adam_state(n, dtype, amsgrad, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(p=(torch.randn(n, generator=g) * 0.05).cuda(), m=torch.zeros(n, device="cuda"), v=torch.zeros(n, device="cuda"),
                vmax=torch.zeros(n, device="cuda") if amsgrad else None,
                grads=[(torch.randn(n, generator=g) * 0.02).to(dtype).cuda() for _ in range(5)])


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("amsgrad,wd", [(False, 0.0), (True, 0.01)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [4096 * 3, 9, 23, 2])
def test_guarded_adam_equals_the_scaled_step_and_a_skip_stores_nothing(amsgrad, wd, dtype, n):
    from kvq import nnops
    c = 0.37
    state = nnops.new_step_state("cuda")
    runs = []
    for guarded in (False, True):
        s = _adam_state(n, dtype, amsgrad, seed=n)
        shadow = s["p"].to(torch.bfloat16)
        state.zero_()
        for g in s["grads"]:
            nnops.step_state_advance(state, 1e-3, 0.1, [], 0.9, 0.999)
            if guarded:
                nnops.adam_step_dev(s["p"], g, s["m"], s["v"], state, weight_decay=wd, vmax=s["vmax"], shadow=shadow, guard=_guard_with(c))
            else:
                nnops.adam_step_dev(s["p"], g, s["m"], s["v"], state, weight_decay=wd, vmax=s["vmax"], shadow=shadow, grad_scale=c)
        torch.cuda.synchronize()
        runs.append((s, shadow))
    (a, sa), (b, sb) = runs
    for k in ("p", "m", "v") + (("vmax",) if amsgrad else ()):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert torch.equal(_bits(sa), _bits(sb))
    assert not torch.equal(a["p"], _adam_state(n, dtype, amsgrad, seed=n)["p"])            # the steps did move the weights
    # skip set: five more steps leave every buffer as it is
    before = {k: b[k].clone() for k in ("p", "m", "v") + (("vmax",) if amsgrad else ())}
    shadow_before = sb.clone()
    skip = _guard_with(coef=0.0, skip=1)
    for g in b["grads"]:
        nnops.step_state_advance(state, 1e-3, 0.1, [], 0.9, 0.999)
        nnops.adam_step_dev(b["p"], g, b["m"], b["v"], state, weight_decay=wd, vmax=b["vmax"], shadow=sb, guard=skip)
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(_bits(t), _bits(b[k])), k
    assert torch.equal(_bits(shadow_before), _bits(sb))


def test_guarded_adam_with_the_fp8_mirror():
    """kvq_adam_step_guarded_fp8 (segment tables as in tests/test_fp8_gpu.py): coef 1 gives the bytes of kvq_adam_step_dev_fp8, a skip
    leaves the mirror, the weights, the moments and the shadow as they are."""
    from kvq import nnops
    from kvq._ffi import check, lib, stream_ptr
    from kvq.engine import fp8_span_table
    n = 6 * 2048 + 512
    segs = [(16, 2048), (2064 + 496, 4096 + 1024), (11 * 1024, 1024)]
    gen = torch.Generator().manual_seed(3)
    p0 = (torch.randn(n, generator=gen) * 0.05).cuda()
    grad = (torch.randn(n, generator=gen) * 0.01).to(torch.bfloat16).cuda()
    off = torch.tensor([o for o, _ in segs], dtype=torch.int64, device="cuda")
    cnt = torch.tensor([c for _, c in segs], dtype=torch.int64, device="cuda")
    scale = torch.tensor([300.0, 2000.0, 900.0], device="cuda")
    span = torch.from_numpy(fp8_span_table([o for o, _ in segs], [c for _, c in segs], n)).cuda()
    state = nnops.new_step_state("cuda")
    nnops.step_state_advance(state, 1e-3, 0.1, [], 0.9, 0.999)

    def run(guard, bufs=None):
        p, m, v, shadow, w8 = bufs or (p0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), p0.to(torch.bfloat16),
                                       torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda"))
        args = (p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), None, shadow.data_ptr(), n, 1, state.data_ptr(), 0.9, 0.999, 1e-8,
                0.0, 1.0, w8.data_ptr(), span.data_ptr(), scale.data_ptr(), off.data_ptr(), cnt.data_ptr(), len(segs), 0)
        if guard is None:
            check(lib().kvq_adam_step_dev_fp8(*args, stream_ptr()), "kvq_adam_step_dev_fp8")
        else:
            check(lib().kvq_adam_step_guarded_fp8(*args, guard.data_ptr(), stream_ptr()), "kvq_adam_step_guarded_fp8")
        torch.cuda.synchronize()
        return p, m, v, shadow, w8

    plain, guarded = run(None), run(_guard_with(1.0))
    for a, b in zip(plain, guarded):
        assert torch.equal(_bits(a) if a.dtype != torch.uint8 else a, _bits(b) if b.dtype != torch.uint8 else b)
    assert bool((guarded[4] != 0xAB).any())                          # the mirror was written
    before = [t.clone() for t in guarded]
    after = run(_guard_with(0.0, skip=1), guarded)
    for a, b in zip(before, after):
        assert torch.equal(_bits(a) if a.dtype != torch.uint8 else a, _bits(b) if b.dtype != torch.uint8 else b)
