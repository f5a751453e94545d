"""The generation kernels of csrc/kvq_generate.hip, one by one: kvq_gen_attn against an f64 softmax(q k^T / 8) v under a derived
per-element bound (tests/_gen_ref.py), with bitwise checks of everything it must and must not write; kvq_gen_embed against the
bits of kvq_embed_ln_fwd; kvq_gen_select against torch.argmax, its bookkeeping against a host restatement, its sampling against
softmax(logits / tau) within five binomial standard deviations; kvq_gen_advance.

Every kernel reads the position t from the generation state on the device: the tests set it there.
"""
import pytest
import torch

import _gen_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                                  # elements of sentinel in front of and behind every buffer (a multiple of 16 bytes)
KEYS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128]
SHAPES = [(1, 1), (5, 3), (8, 12)]
DTYPES = [torch.bfloat16, torch.float32]


def framed(shape, dtype, gen=None, fill=None):
    """(whole, view): `view` of the given shape inside a flat buffer with GUARD sentinel elements on both sides"""
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * GUARD,), -7.0 if dtype.is_floating_point else -7, dtype=dtype, device="cuda")
    view = whole[GUARD:GUARD + n].view(*shape)
    if gen is not None:
        view.copy_(torch.randn(shape, generator=gen, dtype=torch.float32).to(dtype))
    elif fill is not None:
        view.fill_(fill)
    return whole, view


def guards_intact(whole):
    return bool((whole[:GUARD] == -7).all()) and bool((whole[-GUARD:] == -7).all())


def state(t, P=1, Lmax=128, eos=None, pad=0, tau=0.0, seed=0):
    from kvq import nnops
    return nnops.new_gen_state("cuda", t, P, Lmax, eos, pad, temperature=tau, seed=seed)


# ---------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,nh", SHAPES)
def test_gen_attn_self_appends_row_t_and_attends_over_the_cache(B, nh, dtype):
    from kvq import nnops
    H = nh * 64
    g = torch.Generator().manual_seed(100 * B + nh)
    worst = {}
    for n in KEYS:
        t = n - 1
        qkv_w, qkv = framed((B, 3 * H), dtype, g)
        cache_w, cache = framed((B, 128, 2 * H), dtype, g)
        out_w, out = framed((B, H + 64), dtype, fill=3.0)          # 64 columns beside the heads' range: never written
        before = cache_w.clone()
        st = state(t)
        nnops.gen_attn_self(st, qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], cache, nh, out=out[:, :H])
        torch.cuda.synchronize()
        # --- what was written, bit for bit ---
        assert torch.equal(cache[:, t, :H], qkv[:, H:2 * H]) and torch.equal(cache[:, t, H:], qkv[:, 2 * H:]), n
        after = cache_w.clone()
        after[GUARD:-GUARD].view(B, 128, 2 * H)[:, t] = before[GUARD:-GUARD].view(B, 128, 2 * H)[:, t]
        assert torch.equal(after, before), f"n={n}: the cache changed outside row t"
        assert guards_intact(cache_w) and guards_intact(qkv_w) and guards_intact(out_w), n
        assert bool((out[:, H:] == 3.0).all()), n
        assert nnops.read_gen_state(st)["t"] == t
        # --- the values ---
        ref, term = R.attn_ref(R.heads(qkv[:, :H], nh), R.heads(cache[:, :n, :H], nh), R.heads(cache[:, :n, H:], nh))
        ok, worst[n] = R.attn_judge(R.heads(out[:, :H], nh), ref, term, dtype)
        assert ok, f"n={n}: worst |got - ref| / bound = {worst[n]:.3f}"
    print(f"\n[gen_attn self {dtype} B={B} nh={nh}] worst error / bound per key count: " + ", ".join(f"{n}: {w:.3f}" for n, w in worst.items()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,nh", SHAPES)
def test_gen_attn_cross_reads_a_layers_slice_of_the_projection(B, nh, dtype):
    from kvq import nnops
    H = nh * 64
    g = torch.Generator().manual_seed(200 * B + nh)
    worst = {}
    for Se in (1, 12, 128):
        proj_w, proj = framed((B * Se, 3 * 2 * H), dtype, g)       # three layers' keys | values side by side
        q_w, q = framed((B, H), dtype, g)
        out_w, out = framed((B, H), dtype, fill=3.0)
        before = proj_w.clone()
        st = state(5)                                              # (the position plays no part without append)
        kv = proj[:, 2 * H:4 * H]                                   # layer 1
        nnops.gen_attn_cross(st, q, kv, Se, nh, out=out)
        torch.cuda.synchronize()
        assert torch.equal(proj_w, before) and guards_intact(out_w) and guards_intact(q_w)
        kv3 = kv.reshape(B, Se, 2 * H)
        ref, term = R.attn_ref(R.heads(q, nh), R.heads(kv3[:, :, :H], nh), R.heads(kv3[:, :, H:], nh))
        ok, worst[Se] = R.attn_judge(R.heads(out, nh), ref, term, dtype)
        assert ok, f"Se={Se}: worst |got - ref| / bound = {worst[Se]:.3f}"
    print(f"\n[gen_attn cross {dtype} B={B} nh={nh}] worst error / bound per key count: " + ", ".join(f"{n}: {w:.3f}" for n, w in worst.items()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_gen_attn_reads_the_position_from_the_device_state(dtype):
    """the SAME launch arguments, two values of t on the device: two key counts"""
    from kvq import nnops
    B, nh = 5, 3
    H = nh * 64
    g = torch.Generator().manual_seed(7)
    _, qkv = framed((B, 3 * H), dtype, g)
    _, cache = framed((B, 128, 2 * H), dtype, g)
    _, out = framed((B, H), dtype, fill=0.0)
    st = state(0)
    args = (st, qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], cache, nh)
    outs = {}
    for t in (3, 40):
        st[0:1].fill_(t)
        nnops.gen_attn_self(*args, out=out)
        ref, term = R.attn_ref(R.heads(qkv[:, :H], nh), R.heads(cache[:, :t + 1, :H], nh), R.heads(cache[:, :t + 1, H:], nh))
        ok, w = R.attn_judge(R.heads(out, nh), ref, term, dtype)
        assert ok, f"t={t}: {w:.3f}"
        outs[t] = out.clone()
    assert not torch.equal(outs[3], outs[40])


def test_gen_attn_refuses_what_it_cannot_read():
    from kvq import nnops
    from kvq._ffi import KvqError
    st = state(0)
    q = torch.zeros((2, 64), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(KvqError):
        nnops.gen_attn_cross(st, q, torch.zeros((2 * 129, 128), dtype=torch.bfloat16, device="cuda"), 129, 1)      # more than 128 keys
    with pytest.raises(KvqError):
        nnops.gen_attn_self(st, q, q, q, torch.zeros((2, 129, 128), dtype=torch.bfloat16, device="cuda"), 1)      # Smax > 128
    with pytest.raises(KvqError):
        nnops.gen_attn_self(st, q, q, q, torch.zeros((2, 16, 128), dtype=torch.float32, device="cuda"), 1)        # another dtype
    # a position outside the cache stores nothing
    cache_w, cache = framed((2, 16, 128), torch.bfloat16, fill=1.0)
    out_w, out = framed((2, 64), torch.bfloat16, fill=3.0)
    nnops.gen_attn_self(state(16), q, q, q, cache, 1, out=out)
    torch.cuda.synchronize()
    assert bool((cache == 1.0).all()) and bool((out == 3.0).all()) and guards_intact(cache_w) and guards_intact(out_w)


# ---------------------------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("H", [128, 768, 1024, 1536])
def test_gen_embed_has_the_bits_of_embed_ln_fwd(H, dtype):
    from kvq import nnops
    B, S, V = 5, 64, 97
    g = torch.Generator().manual_seed(H)
    word = torch.randn((V, H), generator=g).to(dtype).cuda()
    pos = torch.randn((S, H), generator=g).to(dtype).cuda()
    typ = torch.randn((2, H), generator=g).to(dtype).cuda()
    gamma = (1.0 + 0.1 * torch.randn(H, generator=g)).cuda()
    beta = (0.1 * torch.randn(H, generator=g)).cuda()
    ids = torch.randint(0, V, (B, S), generator=g).cuda()
    full = nnops.embed_ln_fwd(ids.reshape(-1), word, pos, typ[0], gamma, beta, 1e-12, S)[0].view(B, S, H)
    for t in (0, 1, 63):
        out_w, out = framed((B, H), dtype, fill=3.0)
        nnops.gen_embed(state(t, Lmax=S), ids, word, pos, typ[0], gamma, beta, 1e-12, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, full[:, t]), f"t={t}"
        assert guards_intact(out_w)
    out_w, out = framed((B, H), dtype, fill=3.0)
    nnops.gen_embed(state(S, Lmax=S), ids, word, pos, typ[0], gamma, beta, 1e-12, out=out)      # a position outside the buffers
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())


# ---------------------------------------------------------------------------------------------------------------- selection
def sel_buffers(B, Lmax, fill=0):
    ids_w, ids = framed((B, Lmax), torch.int64, fill=fill)
    fin_w, fin = framed((B,), torch.int32, fill=0)
    len_w, lens = framed((B,), torch.int32, fill=Lmax)
    return (ids_w, fin_w, len_w), ids, fin, lens


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("V,ld", [(5, 8), (2048, 2048), (30522, 30528)])
def test_gen_select_greedy_is_the_first_argmax_below_V(V, ld, B, dtype):
    from kvq import nnops
    g = torch.Generator().manual_seed(V + B)
    x = torch.randn((B, ld), generator=g)
    x[:, V:] = 1e30                                                 # the padding columns must never win
    hi = x[:, :V].max() + 1.0
    x[0, [V - 1, V // 2]] = hi                                      # a duplicated maximum: the lower index wins
    if B > 1:
        x[1, [0, V // 3]] = float("nan")                            # NaNs at places that must not win
        x[2, 0] = hi
        x[2, V - 1] = hi
        x[3, :V] = 0.25                                             # a whole row of ties
    whole, logits = framed((B, ld), dtype)
    logits.copy_(x.to(dtype))
    lw, step_logits = framed((B, 4, V), torch.float32, fill=0.0)
    frames, ids, fin, lens = sel_buffers(B, 4, fill=9)
    nnops.gen_select(state(1, Lmax=4), logits, V, ids, fin, lens, step_logits=step_logits)
    torch.cuda.synchronize()
    seen = logits[:, :V].float().cpu()
    want = torch.where(seen.isnan(), torch.full_like(seen, float("-inf")), seen).argmax(dim=1)
    assert ids[:, 2].cpu().tolist() == want.tolist()
    assert want[0] == V // 2 and (B == 1 or (want[2] == 0 and want[3] == 0))
    assert bool((ids[:, [0, 1, 3]] == 9).all()) and not bool(fin.any()) and bool((lens == 4).all())
    got = step_logits[:, 1].cpu()
    assert torch.equal(torch.nan_to_num(got, nan=123.0), torch.nan_to_num(seen, nan=123.0))      # the step's logits row, as f32
    assert bool((step_logits[:, [0, 2, 3]] == 0).all())
    assert all(guards_intact(w) for w in frames + (whole, lw))


@pytest.mark.parametrize("eos", [5, None])
def test_gen_select_bookkeeping_prompt_end_token_and_pads(eos):
    from kvq import nnops
    B, V, Lmax, P, pad = 4, 16, 8, 3, 0
    frames, ids, fin, lens = sel_buffers(B, Lmax, fill=pad)
    prompt = torch.tensor([[11, 12, 13]] * B)
    ids[:, :P] = prompt.cuda()
    # the choice of sentence b at step t; sentence 1 chooses the end token at t = 3, sentence 2 at t = 6 (the last step)
    plan = torch.tensor([[(3 * t + b) % 4 + 6 for t in range(Lmax - 1)] for b in range(B)])
    plan[1, 3], plan[2, 6] = 5, 5
    plan[:, :2] = 5                                                 # inside the prompt an end token changes nothing
    st = state(0, P=P, Lmax=Lmax, eos=eos, pad=pad)
    h_ids, h_fin, h_len = ids.cpu().clone(), torch.zeros(B, dtype=torch.int32), torch.full((B,), Lmax, dtype=torch.int32)
    for t in range(Lmax - 1):
        logits = torch.zeros((B, V), dtype=torch.float32)
        logits[torch.arange(B), plan[:, t]] = 1.0
        nnops.gen_select(st, logits.cuda(), V, ids, fin, lens)
        nnops.gen_advance(st)
        R.select_ref(plan[:, t], h_ids, h_fin, h_len, t, P, eos, pad)
    torch.cuda.synchronize()
    assert nnops.read_gen_state(st) == dict(t=Lmax - 1, P=P, Lmax=Lmax, eos_id=-1 if eos is None else eos, pad_id=pad, seed=0, inv_tau=0.0)
    assert torch.equal(ids.cpu(), h_ids) and torch.equal(fin.cpu(), h_fin) and torch.equal(lens.cpu(), h_len)
    assert torch.equal(ids[:, :P].cpu(), prompt)                    # the prompt is kept
    if eos is None:
        assert not bool(fin.any()) and bool((lens == Lmax).all()) and torch.equal(ids[:, P:].cpu(), plan[:, P - 1:])
    else:
        assert fin.cpu().tolist() == [0, 1, 1, 0] and lens.cpu().tolist() == [Lmax, 5, 8, Lmax]
        assert ids[1].cpu().tolist() == [11, 12, 13, int(plan[1, 2]), 5, pad, pad, pad]
    # one step too many: t + 1 == Lmax stores nothing
    nnops.gen_select(st, torch.zeros((B, V), device="cuda"), V, ids, fin, lens)
    torch.cuda.synchronize()
    assert torch.equal(ids.cpu(), h_ids) and all(guards_intact(w) for w in frames)


@pytest.mark.parametrize("tau", [1.0, 0.5])
def test_gen_select_sampling_draws_from_the_softmax_at_the_temperature(tau):
    from kvq import nnops
    N, V = 8192, 8
    row = torch.tensor([0.0, 1.0, -1.0, 2.0, 0.5, -2.0, 1.5, 0.25])
    logits = row.repeat(N, 1).cuda()
    p = torch.softmax(row.double() / tau, dim=0)

    _, ids, fin, lens = sel_buffers(N, 4)
    st = state(0, Lmax=4)

    def draw(t, seed):
        # temperature and seed travel in the state, as t does: the SAME launch arguments for every draw
        st.copy_(state(t, Lmax=4, tau=tau, seed=seed))
        nnops.gen_select(st, logits, V, ids, fin, lens)
        return ids[:, t + 1].cpu()

    a = draw(0, 1234)
    freq = torch.bincount(a, minlength=V).double() / N
    dev = (freq - p).abs() / R.frequency_bound(p, N)
    print(f"\n[gen_select sampling tau={tau}] frequency deviation / (5 sigma) per class: " + ", ".join(f"{d:.3f}" for d in dev.tolist()))
    assert bool((dev <= 1.0).all())
    assert torch.equal(a, draw(0, 1234))                            # the same (seed, t): the same bits
    assert not torch.equal(a, draw(1, 1234)) and not torch.equal(a, draw(0, 1235))
    assert not torch.equal(a, draw(0, 1234 + (1 << 32)))            # the high word of the seed is part of the key
    st.copy_(state(0, Lmax=4, tau=0.0, seed=1234))                  # temperature 0 in the state: the arg-max, no noise
    nnops.gen_select(st, logits, V, ids, fin, lens)
    assert bool((ids[:, 1] == int(row.argmax())).all())


def test_gumbel_noise_is_finite_for_every_bit_pattern():
    """g = -log(-log u), u = ((bits >> 9) + 1/2) 2^-23: the extreme patterns of the 23-bit uniform (an infinite g would win the
    arg-max whatever its logit) and a million random ones, against f64.  Tolerance: -log u carries logf's 2 ulp (2^-22 relative),
    which -log turns into 2^-22 absolute; plus 2 ulp of g itself, |g| < 17: 2^-22 + 17 * 2^-22 < 2^-17."""
    from kvq import nnops
    edge = torch.arange(4096, dtype=torch.int64)
    ks = torch.cat([edge, (1 << 23) - 1 - edge, (1 << 22) + edge - 2048])          # smallest, largest, middle values of bits >> 9
    bits = torch.cat([ks << 9, (ks << 9) | 0x1FF, torch.tensor([0, 0xFFFFFFFF, 0xFFFFFF00, 0xFFFFFE00, 0x7FFFFFFF, 0x80000000]),
                      torch.randint(0, 1 << 32, (1 << 20,), generator=torch.Generator().manual_seed(3))])
    g = nnops.gen_gumbel_debug(bits.cuda()).cpu().double()
    u = ((bits >> 9).double() + 0.5) * 2.0 ** -23
    assert bool((u > 0).all()) and bool((u < 1).all())
    want = -torch.log(-torch.log(u))
    assert bool(torch.isfinite(g).all())
    assert float(g.min()) >= -2.82 and float(g.max()) <= 16.7
    err = float((g - want).abs().max())
    print(f"\n[gen_select noise] {bits.numel()} bit patterns: g in [{float(g.min()):.4f}, {float(g.max()):.4f}], max |g - f64| = {err:.3e}")
    assert err <= 2.0 ** -17


def test_gen_advance_moves_t_alone():
    from kvq import nnops
    seed = (1 << 63) + 5
    st = state(0, P=3, Lmax=20, eos=102, pad=7, tau=0.5, seed=seed)
    for t in (1, 2):
        nnops.gen_advance(st)
        assert nnops.read_gen_state(st) == dict(t=t, P=3, Lmax=20, eos_id=102, pad_id=7, seed=seed, inv_tau=2.0)
