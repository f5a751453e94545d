"""The gradient-accumulation kernels (csrc/kvq_accum.hip, include/kvq.h "gradient accumulation"): kvq_grad_accumulate bit for bit
against the same sequence of torch f32 operations, and the accumulation state kvq_accum_advance walks."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
# 1 .. 9: the scalar tail alone, one 8-element chunk, chunk + tail; 2056 = 257 chunks: a second workgroup; 5 000 011 is beyond
# 2048 workgroups x 256 threads x 8 elements: the grid-stride loop (with its two-chunk pass) and a 3-element tail
SIZES = [1, 7, 8, 9, 2056, 5_000_011]
CANARY = 8


def _gradients(n, dtype, A, seed):
    """A fresh random gradient per micro-step, magnitudes spread over six decades (small addends must survive in f32)."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = []
    for _ in range(A):
        g = torch.randn(n, generator=gen, device="cuda") * torch.pow(10.0, -6.0 * torch.rand(n, generator=gen, device="cuda"))
        out.append(g.to(dtype))
    return out


def _run_cycle(gs, A):
    """A calls with kvq_accum_advance between them on an accumulator pre-filled with NaN, eight canary elements behind it."""
    from kvq import nnops
    n = gs[0].numel()
    buf = torch.full((n + CANARY,), float("nan"), dtype=torch.float32, device="cuda")
    canary = torch.arange(1, CANARY + 1, dtype=torch.int32, device="cuda") * 0x01010101
    buf[n:] = canary.view(torch.float32)
    state = nnops.new_accum_state("cuda")
    for g in gs:
        nnops.grad_accumulate(g, buf[:n], state, A)
        nnops.accum_advance(state, A)
    torch.cuda.synchronize()
    assert torch.equal(buf[n:].view(torch.int32), canary), "the elements behind n were written"
    assert nnops.read_accum_state(state) == (A, 0)
    return buf[:n].clone()


def _expected(gs, A):
    acc = gs[0].float()
    for g in gs[1:]:
        acc = acc + g.float()
    return acc * torch.tensor(1 / A, dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("A", [1, 2, 3])
def test_accumulate_is_the_sequential_f32_sum_times_one_over_a(dtype, A):
    for n in SIZES:
        gs = _gradients(n, dtype, A, seed=1000 * A + n % 997)
        got, again, want = _run_cycle(gs, A), _run_cycle(gs, A), _expected(gs, A)
        assert not torch.isnan(got).any(), (n, "a NaN of the pre-filled accumulator survived the first micro-step")
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero().flatten()
        assert bad.numel() == 0, (n, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
        assert torch.equal(got.view(torch.int32), again.view(torch.int32)), n


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_positions_inside_a_cycle(dtype):
    """A = 3, state set by hand: position 0 stores (NaN in the accumulator is not read), position 1 adds and does not scale,
    position 2 adds and scales -- each against torch, bit for bit; the state is only read."""
    from kvq import nnops
    n = 2056 + 5
    g = _gradients(n, dtype, 1, seed=5)[0]
    old = torch.randn(n, device="cuda")
    third = torch.tensor(1 / 3, dtype=torch.float32, device="cuda")
    for micro, want in ((0, g.float()), (1, old + g.float()), (2, (old + g.float()) * third)):
        state = nnops.new_accum_state("cuda")
        state[0], state[1] = 7 * 3 + micro, micro
        acc = torch.full((n,), float("nan"), device="cuda") if micro == 0 else old.clone()
        nnops.grad_accumulate(g, acc, state, 3)
        torch.cuda.synchronize()
        assert torch.equal(acc.view(torch.int32), want.view(torch.int32)), micro
        assert nnops.read_accum_state(state) == (7 * 3 + micro, micro)


def test_a_non_finite_gradient_poisons_the_cycle_and_the_next_cycle_is_clean():
    from kvq import nnops
    n, A = 2056, 2
    gs = _gradients(n, torch.bfloat16, 4, seed=9)
    gs[0][77] = float("inf")
    gs[1][77] = float("-inf")
    acc = torch.zeros(n, device="cuda")
    state = nnops.new_accum_state("cuda")
    for g in gs[:2]:
        nnops.grad_accumulate(g, acc, state, A)
        nnops.accum_advance(state, A)
    assert torch.isnan(acc[77]) and torch.isfinite(acc).sum().item() == n - 1       # inf + -inf
    for g in gs[2:]:
        nnops.grad_accumulate(g, acc, state, A)
        nnops.accum_advance(state, A)
    want = (gs[2].float() + gs[3].float()) * torch.tensor(0.5, device="cuda")
    assert torch.equal(acc.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("A", [1, 2, 3])
def test_advance_walks_tick_and_micro(A):
    from kvq import nnops
    state = nnops.new_accum_state("cuda")
    assert nnops.read_accum_state(state) == (0, 0)
    for k in range(1, 2 * A + 2):
        nnops.accum_advance(state, A)
        assert nnops.read_accum_state(state) == (k, k % A), k
    assert int(state.cpu()[1]) >> 32 == 0                       # the padding word stays zero


def test_wrapper_refuses_mismatched_tensors():
    from kvq import nnops
    from kvq._ffi import KvqError
    state = nnops.new_accum_state("cuda")
    g = torch.zeros(16, dtype=torch.bfloat16, device="cuda")
    for acc in (torch.zeros(15, device="cuda"), torch.zeros(16, dtype=torch.bfloat16, device="cuda"), torch.zeros(32, device="cuda")[::2]):
        with pytest.raises(KvqError, match="accumulator"):
            nnops.grad_accumulate(g, acc, state, 2)
    with pytest.raises(KvqError, match="kvq_grad_accumulate"):
        nnops.grad_accumulate(g, torch.zeros(16, device="cuda"), state, 0)
    with pytest.raises(KvqError):
        nnops.grad_accumulate(g.to(torch.float16), torch.zeros(16, device="cuda"), state, 2)
