"""The weight-EMA kernels (csrc/kvq_weight_ema.hip, include/kvq.h "exponential moving average of the trained weights") bit for bit
against their numpy restatement (tests/_weight_ema_ref.py): the update at t = 0 / 1 / 5 / 10^6 with and without a gradient guard,
the state kvq_weight_ema_advance walks, the skipped step, the swap with and without a bf16 shadow, and every refusal.  A NaN the
arithmetic produces has no fixed sign or payload (inf - inf is 0x7fc00000 on the device, 0xffc00000 on an x86 host): the comparisons
let a NaN match any NaN and are exact everywhere else."""
import numpy as np
import pytest
import torch

import _weight_ema_ref as R

pytestmark = pytest.mark.gpu

DECAY = 0.999
# 1 .. 5: the scalar tail alone, one 4-element chunk, chunk + tail; 255 / 257: around one workgroup's worth of lanes; the last one
# is beyond ONE sweep of the update kernel's grid (2048 workgroups x 256 threads x 4 elements x the two chunks a thread has in
# flight = 4 194 304 elements): 257 chunks are left to the second pass of the stride loop and one element to the scalar tail
SWEEP = 2048 * 256 * 4 * 2
SIZES = [1, 3, 4, 5, 255, 257, SWEEP + 4 * 257 + 1]
CANARY = 8
SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -3e-40, np.finfo(np.float32).max, -np.finfo(np.float32).max,
                     np.inf, -np.inf, np.nan, 1.0, -1.5, 1.1754944e-38, 3.0e-5], dtype=np.float32)


def _operands(n, seed):
    """Random p / ema with magnitudes spread over six decades, the first elements replaced by every pair of SPECIALS that fits."""
    rng = np.random.default_rng(seed)
    draw = lambda: (rng.standard_normal(n) * 10.0 ** (-6.0 * rng.random(n))).astype(np.float32)
    p, ema = draw(), draw()
    pp, ee = np.meshgrid(SPECIALS, SPECIALS)
    k = min(n, pp.size)
    p[:k], ema[:k] = pp.reshape(-1)[:k], ee.reshape(-1)[:k]
    return p, ema


def _guard(skip):
    from kvq import nnops
    if skip is None:
        return None
    g = nnops.new_grad_guard("cuda")
    g[2] = int(skip)                                   # struct { double sumsq; float norm, coef; uint32 skip, pad; uint64 skipped; }
    return g


def _with_canary(x):
    """x on the device with CANARY words behind it that no kernel may touch: (view of the first n, whole buffer, canary)."""
    n = x.size
    buf = torch.empty(n + CANARY, dtype=torch.float32, device="cuda")
    buf[:n] = torch.from_numpy(x).cuda()
    canary = torch.arange(1, CANARY + 1, dtype=torch.int32, device="cuda") * 0x01010101
    buf[n:] = canary.view(torch.float32)
    return buf[:n], buf, canary


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def _assert_same(got, want, what):
    bad = R.same_bits(got, want)
    g, w = np.asarray(got), np.asarray(want)
    assert bad.size == 0, (what, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


@pytest.mark.parametrize("skip", [None, 0], ids=["no_guard", "guard_skip0"])
@pytest.mark.parametrize("t", [0, 1, 5, 10 ** 6])
def test_update_is_the_restatement(t, skip):
    from kvq import nnops
    guard = _guard(skip)
    for n in SIZES:
        p, ema0 = _operands(n, seed=100 * (t % 97) + n % 89)
        if t == 0:
            ema0 = np.full(n, np.nan, dtype=np.float32)               # the storing update does not read it: no NaN may survive
        want = R.update(p, ema0, t, DECAY)
        results = []
        for _ in range(2):
            ema, buf, canary = _with_canary(ema0)
            state = nnops.new_weight_ema_state("cuda")
            state[0] = t
            nnops.weight_ema_update(torch.from_numpy(p).cuda(), ema, state, DECAY, guard=guard)
            torch.cuda.synchronize()
            assert torch.equal(buf[n:].view(torch.int32), canary), (n, "the elements behind n were written")
            assert nnops.read_weight_ema_state(state) == (t, 0.0), "the update only reads the state"
            results.append(ema.cpu().numpy())
        _assert_same(results[0], want, (t, n))
        if t == 0:
            assert np.array_equal(results[0].view(np.uint32), p.view(np.uint32)), (n, "the first update is a copy of p, NaN payloads included")
        assert np.array_equal(results[0].view(np.uint32), results[1].view(np.uint32)), (t, n, "two runs differ")


@pytest.mark.parametrize("t", [0, 5])
def test_a_skipped_step_changes_no_byte(t):
    from kvq import nnops
    guard = _guard(1)
    guard_before = guard.clone()
    for n in (5, 257, 2048 * 256 * 4 + 7):
        p, ema0 = _operands(n, seed=7 + n % 13)
        ema, buf, canary = _with_canary(ema0)
        state = nnops.new_weight_ema_state("cuda")
        state[0], state[1] = t, int(np.float32(0.25).view(np.uint32))
        before = state.clone()
        nnops.weight_ema_update(torch.from_numpy(p).cuda(), ema, state, DECAY, guard=guard)
        nnops.weight_ema_advance(state, DECAY, guard=guard)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(ema), ema0.view(np.uint32)), (t, n, "a skipped update stored something")
        assert torch.equal(buf[n:].view(torch.int32), canary)
        assert torch.equal(state, before), "a skipped step moved the state"
    assert torch.equal(guard, guard_before), "the guard is only read"


@pytest.mark.parametrize("skip", [None, 0], ids=["no_guard", "guard_skip0"])
def test_advance_walks_the_state(skip):
    from kvq import nnops
    guard = _guard(skip)
    state = nnops.new_weight_ema_state("cuda")
    want = (0, 0.0)
    assert nnops.read_weight_ema_state(state) == want
    for _ in range(12):
        nnops.weight_ema_advance(state, DECAY, guard=guard)
        want = R.advance(want, DECAY)
        assert nnops.read_weight_ema_state(state) == want
    assert want[0] == 12 and want[1] == float(np.float32(np.float64(12.0) / np.float64(21.0)))
    for t in (10 ** 6, 2 ** 40):
        state[0] = t
        nnops.weight_ema_advance(state, DECAY, guard=guard)
        assert nnops.read_weight_ema_state(state) == (t + 1, float(np.float32(DECAY)))           # capped at the decay
    assert int(state.cpu()[1]) >> 32 == 0                       # the padding word stays zero


def test_update_then_advance_over_steps_follows_the_recurrence():
    """The two kernels as the step runs them: six updates of one buffer, the state walked on the device."""
    from kvq import nnops
    n = 1029
    rng = np.random.default_rng(3)
    ema = torch.full((n,), float("nan"), device="cuda")
    state = nnops.new_weight_ema_state("cuda")
    want, st = None, (0, 0.0)
    for step in range(6):
        p = rng.standard_normal(n).astype(np.float32)
        nnops.weight_ema_update(torch.from_numpy(p).cuda(), ema, state, DECAY)
        nnops.weight_ema_advance(state, DECAY)
        want, st = R.update(p, want, st[0], DECAY), R.advance(st, DECAY)
        _assert_same(ema.cpu().numpy(), want, step)
        assert nnops.read_weight_ema_state(state) == st


@pytest.mark.parametrize("shadow", [False, True], ids=["no_shadow", "bf16_shadow"])
def test_swap_exchanges_exactly_and_a_second_swap_restores(shadow):
    from kvq import nnops
    for n in SIZES[:-1] + [2048 * 256 * 4 + 6]:                  # (beyond one sweep of the swap kernel's grid: one chunk per pass)
        p0, e0 = _operands(n, seed=11 + n % 17)
        p, pbuf, canary = _with_canary(p0)
        e, ebuf, _ = _with_canary(e0)
        sh = torch.full((n + CANARY,), 0x1234, dtype=torch.int16, device="cuda").view(torch.bfloat16) if shadow else None
        want_p, want_e, want_sh = R.swap(p0, e0, shadow=shadow)
        nnops.weight_ema_swap(p, e, shadow=sh[:n] if shadow else None)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(p), want_p.view(np.uint32)), (n, "p is not the old average, bit for bit")
        assert np.array_equal(_bits(e), want_e.view(np.uint32)), (n, "the average is not the old p, bit for bit")
        assert torch.equal(pbuf[n:].view(torch.int32), canary) and torch.equal(ebuf[n:].view(torch.int32), canary)
        if shadow:
            got_sh = sh.view(torch.int16).cpu().numpy().view(np.uint16)
            bad = R.same_bits_bf16(got_sh[:n], want_sh)
            assert bad.size == 0, (n, bad[:8].tolist(), got_sh[bad[:8]].tolist(), want_sh[bad[:8]].tolist())
            assert (got_sh[n:] == 0x1234).all(), (n, "the shadow behind n was written")
            # the rounding of the Adam kernels' shadow store is torch's own (nearest even) wherever the value is a number
            ref = torch.from_numpy(want_p).cuda().to(torch.bfloat16).view(torch.int16).cpu().numpy().view(np.uint16)
            assert R.same_bits_bf16(got_sh[:n], ref).size == 0
        nnops.weight_ema_swap(p, e, shadow=sh[:n] if shadow else None)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(p), p0.view(np.uint32)) and np.array_equal(_bits(e), e0.view(np.uint32)), (n, "the second swap did not restore")
        if shadow:
            assert R.same_bits_bf16(sh.view(torch.int16).cpu().numpy().view(np.uint16)[:n], R.bf16_bits(p0)).size == 0


def test_every_refusal_returns_an_error_and_names_it():
    from kvq import _ffi, nnops
    from kvq._ffi import KvqError
    lib = _ffi.lib()
    buf = torch.zeros(64, device="cuda")
    other = torch.zeros(64, device="cuda")
    sh = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
    state = nnops.new_weight_ema_state("cuda")
    guard = nnops.new_grad_guard("cuda")
    p, q, s, g, h = buf.data_ptr(), other.data_ptr(), state.data_ptr(), guard.data_ptr(), sh.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    err = lambda: lib.kvq_last_error()
    for args in ((None, q, 16, DECAY, s, None, st), (p, None, 16, DECAY, s, None, st), (p, q, 16, DECAY, None, None, st)):
        assert lib.kvq_weight_ema_update(*args) != 0 and b"kvq_weight_ema_update" in err() and b"null" in err()
    for n in (0, -4):
        assert lib.kvq_weight_ema_update(p, q, n, DECAY, s, None, st) != 0 and b"n < 1" in err()
    for d in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert lib.kvq_weight_ema_update(p, q, 16, d, s, g, st) != 0 and b"decay" in err()
        assert lib.kvq_weight_ema_advance(s, d, g, st) != 0 and b"kvq_weight_ema_advance" in err() and b"decay" in err()
    for args in ((p + 4, q, 16, DECAY, s, None, st), (p, q + 8, 16, DECAY, s, None, st), (p, q, 16, DECAY, s + 4, None, st),
                 (p, q, 16, DECAY, s, g + 4, st)):
        assert lib.kvq_weight_ema_update(*args) != 0 and b"aligned" in err()
    assert lib.kvq_weight_ema_update(p, p + 32, 16, DECAY, s, None, st) != 0 and b"overlap" in err()
    assert lib.kvq_weight_ema_advance(None, DECAY, None, st) != 0 and b"null" in err()
    assert lib.kvq_weight_ema_advance(s + 4, DECAY, None, st) != 0 and b"aligned" in err()
    for args in ((None, q, None, 16, st), (p, None, None, 16, st)):
        assert lib.kvq_weight_ema_swap(*args) != 0 and b"kvq_weight_ema_swap" in err() and b"null" in err()
    assert lib.kvq_weight_ema_swap(p, q, None, 0, st) != 0 and b"n < 1" in err()
    assert lib.kvq_weight_ema_swap(p + 8, q, None, 16, st) != 0 and b"aligned" in err()
    assert lib.kvq_weight_ema_swap(p, q, h + 4, 16, st) != 0 and b"aligned" in err()
    assert lib.kvq_weight_ema_swap(p, p, None, 16, st) != 0 and b"overlap" in err()
    assert lib.kvq_weight_ema_swap(p, p + 48, None, 16, st) != 0 and b"overlap" in err()
    assert lib.kvq_weight_ema_swap(p, q, q + 32, 16, st) != 0 and b"shadow" in err()
    torch.cuda.synchronize()
    assert not buf.any() and not other.any() and not sh.any() and not state.any() and not guard.any()       # nothing was launched
    # the Python wrappers: tensors that do not fit each other
    for ema in (torch.zeros(63, device="cuda"), torch.zeros(64, dtype=torch.bfloat16, device="cuda"), torch.zeros(128, device="cuda")[::2]):
        with pytest.raises(KvqError, match="average"):
            nnops.weight_ema_update(buf, ema, state, DECAY)
        with pytest.raises(KvqError, match="average"):
            nnops.weight_ema_swap(buf, ema)
    with pytest.raises(KvqError, match="shadow"):
        nnops.weight_ema_swap(buf, other, shadow=torch.zeros(64, device="cuda"))
    with pytest.raises(KvqError, match="overlap"):
        nnops.weight_ema_swap(buf, buf)
    with pytest.raises(KvqError, match="decay"):
        nnops.weight_ema_update(buf, other, state, 1.0)
