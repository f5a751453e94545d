"""The codebook-revival kernels (csrc/kvq_vq_revive.hip) against the numpy restatement (tests/_revive_ref.py), bit for bit: usage
flags, idle counters, donor rows, and the codebook, moments, EMA statistics and counter after apply.  Every output is pre-filled with a
sentinel so that "not touched" is visible.  Shapes: the smallest at which the kernels take another path (K and N off every block
size, 16-byte and scalar row paths, rows spanning many chunks, one token, several codebooks)."""
import numpy as np
import pytest
import torch

import _revive_ref as R

pytestmark = pytest.mark.gpu

SENT_F = -7.25            # sentinel of float outputs (no encoder output or zero below equals it)
SENT_I = -77              # sentinel of the guard elements around `used`
DEV = "cuda"


def _lib():
    from kvq import _ffi
    return _ffi.lib(), _ffi.check, _ffi.stream_ptr


def _z(G, N, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(G, N, D, generator=g)
    z[:, :, 0] = -0.0                                   # a signed zero among the donors' values
    z = z.to(dtype)
    return z.to(DEV), z.float().numpy()                  # the device tensor and its exact f32 values


def _idx(G, N, K, seed, kind="random"):
    rng = np.random.default_rng(seed)
    if kind == "all_used":
        idx = np.stack([np.resize(rng.permutation(K), max(N, K))[:N] for _ in range(G)])
        assert N >= K
    elif kind == "none_used":
        idx = np.full((G, N), -1)
    else:
        idx = rng.integers(0, K, (G, N))
        idx[:, ::2] = idx[:, ::2] // 3                  # crowd the tokens onto a third of the codes: many stay unused
    return idx.astype(np.int64)


def usage_flags(idx, K, guard=True):
    lib, check, sp = _lib()
    G, N = idx.shape
    buf = torch.full((G * K + 2,), SENT_I, dtype=torch.int32, device=DEV)
    used = buf[1:-1]
    check(lib.kvq_vq_usage_flags(torch.from_numpy(idx).to(DEV).data_ptr(), N, K, G, used.data_ptr(), sp()), "kvq_vq_usage_flags")
    torch.cuda.synchronize()
    assert buf[0].item() == SENT_I and buf[-1].item() == SENT_I, "kvq_vq_usage_flags wrote outside used[G, K]"
    return used.clone().view(G, K)


def select(z, used, idle, T, seed, rank=0, world=1):
    lib, check, sp = _lib()
    G, N, D = z.shape
    K = used.shape[1]
    idle = torch.from_numpy(idle).to(DEV).contiguous()
    rows = torch.full((G, K, D), SENT_F, dtype=torch.float32, device=DEV)
    check(lib.kvq_vq_revive_select(z.data_ptr(), used.contiguous().data_ptr(), N, K, D, G, 1 if z.dtype == torch.bfloat16 else 0, T, seed,
                                   rank, world, idle.data_ptr(), rows.data_ptr(), sp()), "kvq_vq_revive_select")
    torch.cuda.synchronize()
    return idle, rows


def apply(rows, idle, T, E, counter, **opt):
    lib, check, sp = _lib()
    G, K, D = rows.shape
    p = lambda n: opt[n].data_ptr() if opt.get(n) is not None else None
    check(lib.kvq_vq_revive_apply(rows.data_ptr(), K, D, G, T, idle.data_ptr(), E.data_ptr(), p("m"), p("v"), p("vmax"), p("ema_n"), p("ema_m"),
                                  counter.data_ptr(), sp()), "kvq_vq_revive_apply")
    torch.cuda.synchronize()


def _same_bits(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype == np.float32:
        assert np.array_equal(R.bits(got), R.bits(want)), what
    else:
        assert np.array_equal(got, want), what


def _rows_expected(rows_ref, dead):
    """Dead codes: the restatement's row; every other row keeps the sentinel."""
    want = np.full(rows_ref.shape, SENT_F, np.float32)
    want[dead] = rows_ref[dead]
    return want


def _run_case(G, N, K, D, dtype, T, idle0=None, kind="random", seed=1234, optional=("m", "v", "vmax", "ema_n", "ema_m")):
    z, z32 = _z(G, N, D, dtype, seed=G * 1000 + D)
    idx = _idx(G, N, K, seed=N + K, kind=kind)
    idle0 = np.zeros((G, K), np.int32) if idle0 is None else idle0
    used = usage_flags(idx, K)
    used_ref = R.usage_flags(idx, K)
    _same_bits(used, used_ref, "used")
    idle1, rows = select(z, used, idle0, T, seed)
    idle_ref, dead, rows_ref, _owner, _token = R.select([z32], used_ref, idle0, T, seed)
    _same_bits(idle1, idle_ref, "idle after select")
    _same_bits(rows, _rows_expected(rows_ref, dead), "rows")
    # apply: sentinels everywhere, then compare every array
    rng = np.random.default_rng(7)
    host = dict(E=rng.standard_normal((G, K, D)).astype(np.float32))
    for name in ("m", "v", "vmax", "ema_m"):
        host[name] = np.full((G, K, D), SENT_F, np.float32) if name in optional else None
    host["ema_n"] = np.full((G, K), SENT_F, np.float32) if "ema_n" in optional else None
    devt = {k: (torch.from_numpy(a).to(DEV) if a is not None else None) for k, a in host.items()}
    counter = torch.tensor([0, 40], dtype=torch.int64, device=DEV)
    apply(rows, idle1, T, devt["E"], counter, **{k: devt[k] for k in ("m", "v", "vmax", "ema_n", "ema_m")})
    idle2_ref, E_ref, cnt_ref, opt_ref = R.apply(rows_ref, dead, idle_ref, host["E"], (0, 40),
                                                 **{k: host[k] for k in ("m", "v", "vmax", "ema_n", "ema_m")})
    _same_bits(idle1, idle2_ref, "idle after apply")
    _same_bits(devt["E"], E_ref, "E")
    for k in ("m", "v", "vmax", "ema_n", "ema_m"):
        if host[k] is not None:
            _same_bits(devt[k], opt_ref[k], k)
    assert counter.tolist() == [cnt_ref[0], cnt_ref[1]], (counter.tolist(), cnt_ref)
    return dict(dead=dead, rows=rows, idle=idle1, counter=counter, E=devt["E"], z=z, z32=z32, used=used, used_ref=used_ref)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_odd_sizes_one_codebook(dtype):
    """K = 37 and N = 70 fall off every block size; row pitch 160 / 80 bytes; T = 1: unused means dead at once."""
    r = _run_case(1, 70, 37, 40, dtype, T=1)
    assert 0 < r["dead"].sum() < 37


def test_three_codebooks_and_saturation():
    """idle preset to 0, 1, 2, 3 and INT32_MAX with T = 3: the counter saturates, 2 -> 3 dies, 0 and 1 survive."""
    G, K = 3, 64
    idle0 = np.resize(np.array([0, 1, 2, 3, R.INT32_MAX, 2, 0], np.int32), G * K).reshape(G, K)
    r = _run_case(G, 128, K, 32, torch.bfloat16, T=3, idle0=idle0)
    assert 0 < r["dead"].sum() < G * K
    assert r["idle"].max().item() < R.INT32_MAX                # every saturated code was unused-and-dead (reset) or used (reset)


def test_idle_saturates_without_wrapping():
    """idle + 1 saturates at INT32_MAX instead of wrapping to a negative count; T = INT32_MAX: only a saturated code is dead."""
    idle0 = np.array([[R.INT32_MAX, R.INT32_MAX - 1, 5, 0]], np.int32)
    z, z32 = _z(1, 4, 8, torch.float32, 3)
    used = torch.tensor([[0, 0, 0, 1]], dtype=torch.int32, device=DEV)
    idle1, rows = select(z, used, idle0, R.INT32_MAX, 9)
    assert idle1.tolist() == [[R.INT32_MAX, R.INT32_MAX, 6, 0]]
    ref_idle, dead, rows_ref, _, _ = R.select([z32], used.cpu().numpy(), idle0, R.INT32_MAX, 9)
    assert dead.tolist() == [[True, True, False, False]]
    _same_bits(rows, _rows_expected(rows_ref, dead), "rows")


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 36), (torch.float32, 6), (torch.float32, 768), (torch.bfloat16, 768)],
                         ids=["bf16-72B-scalar", "f32-24B-scalar", "f32-768", "bf16-768"])
def test_row_paths(dtype, D):
    """D = 36 in bf16: 72-byte rows, the scalar path; D = 768: a row spans many 16-byte chunks per lane."""
    r = _run_case(2 if D < 100 else 1, 64, 8, D, dtype, T=1, kind="none_used")
    assert r["dead"].all()


def test_one_token():
    r = _run_case(2, 1, 5, 8, torch.bfloat16, T=1)
    dead = r["dead"]
    assert dead.sum() == 2 * 5 - 2                             # each codebook's one token uses one code; all the others take ITS row
    for g in range(2):
        for k in np.nonzero(dead[g])[0]:
            assert np.array_equal(R.bits(r["rows"][g, k].cpu().numpy()), R.bits(r["z32"][g, 0]))


def test_every_code_used_touches_nothing():
    r = _run_case(2, 96, 48, 16, torch.float32, T=1, kind="all_used", idle0=np.full((2, 48), 5, np.int32))
    assert not r["dead"].any() and r["counter"].tolist() == [0, 40]
    assert (r["rows"] == SENT_F).all() and not r["idle"].any()


def test_every_code_dead():
    r = _run_case(1, 70, 37, 40, torch.bfloat16, T=2, kind="none_used", idle0=np.ones((1, 37), np.int32))
    assert r["dead"].all() and r["counter"].tolist() == [37, 77]


def test_indices_outside_the_codebook_are_ignored():
    K = 37
    idx = np.array([[-1, K, 3, K + 100, -5, 2**40, 36, 0, -2**40, 3]], np.int64)
    used = usage_flags(idx, K)                                  # (checks its two guard elements itself)
    want = np.zeros((1, K), np.int32)
    want[0, [0, 3, 36]] = 1
    _same_bits(used, want, "used")
    _same_bits(used, R.usage_flags(idx, K), "used against the restatement")


def test_four_ranks_one_owner_per_code():
    """world = 4, select once per rank on the same inputs: exactly the restatement's owner wrote a row (the others zeros), and the
    sum over the ranks equals the world = 1 rows up to the sign of zero."""
    G, N, K, D, T, seed = 2, 70, 37, 40, 1, 4321
    z, z32 = _z(G, N, D, torch.bfloat16, 11)
    idx = _idx(G, N, K, 5)
    used = usage_flags(idx, K)
    idle0 = np.zeros((G, K), np.int32)
    _idle, rows1 = select(z, used, idle0, T, seed)
    ref_idle, dead, _rows_ref, owner, token = R.select([z32] * 4, R.usage_flags(idx, K), idle0, T, seed)
    assert dead.sum() > 8 and len(set(owner[dead].tolist())) == 4            # every rank owns some code
    per_rank = []
    for rank in range(4):
        idle_r, rows_r = select(z, used, idle0, T, seed, rank=rank, world=4)
        _same_bits(idle_r, ref_idle, f"idle on rank {rank}")
        _, _, want_r, _, _ = R.select([z32] * 4, R.usage_flags(idx, K), idle0, T, seed, rank=rank)
        _same_bits(rows_r, _rows_expected(want_r, dead), f"rows on rank {rank}")
        per_rank.append(rows_r.cpu().numpy())
    for g, k in zip(*np.nonzero(dead)):
        nz = [r for r in range(4) if R.bits(per_rank[r][g, k]).any()]        # (-0.0 has a bit set: the owner's row is never all +0.0)
        assert nz == [owner[g, k]], (g, k, nz, owner[g, k])
    total = per_rank[0] + per_rank[1] + per_rank[2] + per_rank[3]
    one = rows1.cpu().numpy()
    assert np.array_equal(total[dead], one[dead])                             # == : up to the sign of zero
    assert np.array_equal(R.bits(total[dead]), R.bits(one[dead] + np.float32(0.0)))


@pytest.mark.parametrize("missing", ["m", "v", "vmax", "ema_n", "ema_m"])
def test_apply_with_one_optional_pointer_null(missing):
    r = _run_case(2, 40, 24, 12, torch.float32, T=1, optional=tuple(n for n in ("m", "v", "vmax", "ema_n", "ema_m") if n != missing))
    assert r["dead"].any()


def test_two_applies_count_each_call():
    r = _run_case(1, 70, 37, 40, torch.float32, T=1)               # first apply: last = dead, total = 40 + dead; idle is 0 everywhere now
    n1 = int(r["dead"].sum())
    assert r["counter"].tolist() == [n1, 40 + n1] and not r["idle"].any()
    used = torch.ones((1, 37), dtype=torch.int32, device=DEV)
    used[0, :5] = 0
    idle2, rows2 = select(r["z"], used, r["idle"].cpu().numpy(), 1, 99)
    E_before = r["E"].clone()
    apply(rows2, idle2, 1, r["E"], r["counter"])
    assert r["counter"].tolist() == [5, 40 + n1 + 5] and not idle2.any()
    assert torch.equal(r["E"][0, 5:], E_before[0, 5:]) and torch.equal(r["E"][0, :5], rows2[0, :5])
    idle3 = torch.zeros((1, 37), dtype=torch.int32, device=DEV)
    apply(rows2, idle3, 1, r["E"], r["counter"])                    # nothing dead: last goes back to 0 without a clear from outside
    assert r["counter"].tolist() == [0, 40 + n1 + 5]


def test_seed_offset_adds_the_device_step_count():
    from kvq import nnops
    G, N, K, D, T, seed = 1, 70, 37, 40, 1, 1000
    z, _ = _z(G, N, D, torch.bfloat16, 2)
    used = torch.zeros((G, K), dtype=torch.int32, device=DEV)
    idle0 = np.zeros((G, K), np.int32)
    state = nnops.new_step_state(torch.device(DEV))
    state[0] = 5                                                    # the step count is the state's first word
    torch.cuda.synchronize()
    try:
        nnops.set_seed_offset(state)
        _, with_offset = select(z, used, idle0, T, seed)
    finally:
        nnops.set_seed_offset(None)
    _, plain5 = select(z, used, idle0, T, seed + 5)
    _, plain0 = select(z, used, idle0, T, seed)
    assert torch.equal(with_offset, plain5) and not torch.equal(with_offset, plain0)
