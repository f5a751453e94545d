"""The beam-search kernels of csrc/kvq_generate.hip, one by one: kvq_beam_select against the f64 reference of tests/_beam_ref.py
(chosen parents and tokens on decided steps, every score under the derived tolerance, the whole bookkeeping exactly), its tie rule
and its bookkeeping cases; kvq_beam_attn against kvq_gen_attn on a physically gathered cache, BIT FOR BIT; kvq_beam_gather against
the reference.  Every kernel reads the position t from the generation state on the device: the tests set it there.
"""
import numpy as np
import pytest
import torch

import _beam_ref as BR
import _gen_ref as GR
from test_generate_kernels_gpu import GUARD, framed, guards_intact, state

pytestmark = pytest.mark.gpu

INF = float("inf")


def run_select(st, x, V, W, t, P=1, eos=None, pad=0, trace=False):
    """one kvq_beam_select launch on a host state -> (the state after it, step_logits or None, the frames' guards hold)"""
    from kvq import nnops
    R, L = st["ids"].shape
    frames, dev = {}, {}
    for k, v in st.items():
        frames[k], dev[k] = framed(v.shape, torch.from_numpy(v).dtype)
        dev[k].copy_(torch.from_numpy(v))
    lw, logits = framed(tuple(x.shape), x.dtype)
    logits.copy_(x)
    sw, step_logits = framed((R, L, V), torch.float32, fill=0.0) if trace else (None, None)
    nnops.beam_select(state(t, P=P, Lmax=L, eos=eos, pad=pad), logits, V, W, dev["ids"], dev["parent"], dev["scores"], dev["step_scores"],
                      dev["anc"], dev["finished"], dev["lengths"], step_logits=step_logits)
    torch.cuda.synchronize()
    ok = all(guards_intact(w) for w in frames.values()) and guards_intact(lw) and (sw is None or guards_intact(sw))
    return BR.state_from(dev), (None if step_logits is None else step_logits.cpu()), ok


@pytest.mark.parametrize("V,ld,B,W,dtype", BR.select_cases())
def test_beam_select_against_the_f64_reference(V, ld, B, W, dtype):
    old, x, t = BR.select_case(V, ld, B, W, dtype, BR.select_seed(V, W, dtype))
    new, step_logits, ok = run_select(old, x, V, W, t, trace=V <= 2048)
    assert ok
    seen = x.float().numpy()
    decided, worst = BR.judge_step(old, new, seen, V, W, t, 1, None, 0)
    share = 1.0 - sum(decided[:B]) / B
    print(f"\n[beam_select V={V} W={W} {dtype}] worst |s - ref| / tol = {worst:.3f}; undecided sentences {share:.2f}")
    assert share <= 0.05
    if step_logits is not None:                                       # the logits of the live beams, as f32, at row (r, t) alone
        live = [r for r in range(B * W) if not old["finished"][r]]
        assert torch.equal(step_logits[live, t], x[live, :V].float())
        step_logits[live, t] = 0
        assert not bool(step_logits.any())


def tie_state(W, L=4):
    st = BR.new_state(1, W, L, [[3]], 0, R=W)
    st["scores"][:] = np.float32(-1.25)
    return st


def test_beam_select_ties_go_to_the_lower_beam_then_the_lower_token():
    V, W, t = 40, 4, 1
    x = torch.zeros((W, V))
    x[:, [7, 21]] = 2.0                                               # equal logits at two columns of identical rows, identical scores
    x[:, 30] = 1.0
    for dtype in (torch.float32, torch.bfloat16):
        new, _, ok = run_select(tie_state(W), x.to(dtype), V, W, t)
        assert ok
        assert new["parent"][:, t + 1].tolist() == [0, 0, 1, 1] and new["ids"][:, t + 1].tolist() == [7, 21, 7, 21]
        assert len(set(new["scores"].tolist())) == 1
    # a whole row of ties: tokens 0, 1, 2, 3 of beam 0 (the other beams are dead)
    st = tie_state(W)
    st["scores"][1:] = -INF
    new, _, _ = run_select(st, torch.full((W, V), 0.25), V, W, t)
    assert new["parent"][:, t + 1].tolist() == [0] * W and new["ids"][:, t + 1].tolist() == [0, 1, 2, 3]
    # a finished beam ranks as (w, 0): in front of a live candidate of the same score from a later beam, behind one from an earlier
    st = tie_state(2)
    st["finished"][1], st["lengths"][1] = 1, 2
    row = torch.full((2, V), -100.0)
    row[:, 5] = 0.0                                                   # lse = 0 exactly (40 e^-100 vanishes in f64 too): the live beam's best continues at -1.25
    new, _, _ = run_select(st, row, V, 2, t)
    assert new["parent"][:, t + 1].tolist() == [0, 1] and new["ids"][:, t + 1].tolist() == [5, 0]
    assert new["scores"].tolist() == [-1.25, -1.25] and new["finished"].tolist() == [0, 1]
    st["finished"][:], st["lengths"][:] = [1, 0], [2, 4]
    new, _, _ = run_select(st, row, V, 2, t)
    assert new["parent"][:, t + 1].tolist() == [0, 1] and new["ids"][:, t + 1].tolist() == [0, 5] and new["finished"].tolist() == [1, 0]


def test_beam_select_prompt_steps_keep_tokens_parents_and_scores():
    V, W, B, L, P = 64, 3, 2, 8, 4
    g = np.random.default_rng(0)
    old = BR.new_state(B, W, L, g.integers(0, V, (B, P)), 9)
    x = torch.randn((old["ids"].shape[0], V), generator=torch.Generator().manual_seed(0))
    for t in range(P - 1):
        new, logits, ok = run_select(old, x, V, W, t, P=P, pad=9, trace=True)
        assert ok
        BR.judge_step(old, new, x.numpy(), V, W, t, P, None, 9)
        assert np.array_equal(new["ids"], old["ids"]) and np.array_equal(new["scores"], old["scores"])
        assert np.array_equal(new["parent"][:, t + 1], np.arange(old["ids"].shape[0]))
        assert torch.equal(logits[:, t], x)                           # the prompt's logits rows, every row
        old = new
    # t = P - 1, beams 1 .. W-1 dead: W distinct tokens from row 0 of each sentence
    t = P - 1
    new, _, ok = run_select(old, x, V, W, t, P=P, pad=9)
    assert ok
    decided, _ = BR.judge_step(old, new, x.numpy(), V, W, t, P, None, 9)
    assert all(decided)
    for b in range(B):
        rows = slice(b * W, (b + 1) * W)
        assert new["parent"][rows, t + 1].tolist() == [b * W] * W
        assert new["ids"][rows, t + 1].tolist() == x[b * W].topk(W).indices.tolist()
        assert np.all(np.diff(new["scores"][rows]) < 0)
    assert new["finished"][B * W:].tolist() == [1] * (old["ids"].shape[0] - B * W) and np.all(new["scores"][B * W:] == -INF)


def test_beam_select_end_token_finished_beams_nan_rows_and_positions_outside():
    V, W, L, t, eos, pad = 48, 3, 8, 2, 17, 5
    old = BR.new_state(1, W, L, [[3]], pad, R=W)
    old["scores"][:] = [-1.0, -1.5, -2.0]
    old["finished"][1], old["lengths"][1] = 1, 2                       # beam 1 is finished: carried with a pad, its score unchanged
    x = torch.full((W, V), -20.0)
    x[0, eos], x[0, 4] = 3.0, 2.5                                       # beam 0: the end token first, then token 4
    x[2, :] = float("nan")                                              # beam 2: a row of NaNs offers nothing
    new, _, ok = run_select(old, x, V, W, t, eos=eos, pad=pad)
    assert ok
    decided, worst = BR.judge_step(old, new, x.numpy(), V, W, t, 1, eos, pad)
    assert all(decided) and worst <= 1.0
    assert new["parent"][:, t + 1].tolist() == [0, 1, 0] and new["ids"][:, t + 1].tolist() == [eos, pad, 4]
    assert new["finished"].tolist() == [1, 1, 0] and new["lengths"].tolist() == [t + 2, 2, L]
    assert new["scores"][1] == np.float32(-1.5)
    # one NaN among a beam's columns < V is enough; fewer candidates than beams leave dead beams behind
    x2 = x.clone()
    x2[0, 40] = float("nan")
    new2, _, _ = run_select(old, x2, V, W, t, eos=eos, pad=pad)
    BR.judge_step(old, new2, x2.numpy(), V, W, t, 1, eos, pad)
    assert new2["parent"][:, t + 1].tolist() == [1, 1, 2] and new2["scores"].tolist() == [-1.5, -INF, -INF]
    assert new2["finished"].tolist() == [1, 1, 1] and new2["ids"][:, t + 1].tolist() == [pad, pad, pad]
    # a position outside the buffers stores nothing: t + 1 == Lmax, t beyond, t < 0
    for bad in (L - 1, L, 3 * L, -1):
        same, _, ok = run_select(old, x, V, W, bad, eos=eos, pad=pad)
        assert ok and all(np.array_equal(same[k], old[k], equal_nan=True) for k in old), bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_beam_select_three_chained_steps_keep_the_reference_ancestry(dtype):
    """select -> advance three times on the device; the reference follows from the kernel's state after each step"""
    from kvq import nnops
    V, W, B, L, P = 2048, 4, 3, 8, 2
    host = BR.new_state(B, W, L, np.random.default_rng(3).integers(0, V, (B, P)), 0)
    R = host["ids"].shape[0]
    xs = BR.chain_logits(R, V, 4, dtype)
    dev = BR.state_to(host, "cuda")
    st = state(0, P=P, Lmax=L, eos=None, pad=0)
    undecided = 0
    for t in range(4):
        x = xs[t]
        old = BR.state_from(dev)
        nnops.beam_select(st, x.cuda(), V, W, dev["ids"], dev["parent"], dev["scores"], dev["step_scores"], dev["anc"], dev["finished"],
                          dev["lengths"])
        nnops.gen_advance(st)
        new = BR.state_from(dev)
        decided, _ = BR.judge_step(old, new, x.float().numpy(), V, W, t, P, None, 0)
        undecided += B - sum(decided[:B])
    assert undecided == 0                                             # (the seed of chain_logits, checked on the CPU: tests/test_beam_ref.py)
    assert nnops.read_gen_state(st)["t"] == 4
    hyp = nnops.beam_gather(st, dev["ids"], dev["anc"], dev["lengths"]).cpu().numpy()
    assert np.array_equal(hyp, BR.gather_ref(new, 4, 0))
    for r in range(B * W):                                            # the ancestry table says what the parents say
        assert np.array_equal(hyp[r, :5], BR.backtrack(new["ids"], new["parent"], r, 4)), r
        assert new["anc"][0][r, :5].tolist() == slots_of(new["parent"], r, 4)


def slots_of(parent, r, t):
    out = []
    for j in range(t, -1, -1):
        out.append(r)
        r = int(parent[r, j])
    return out[::-1]


def test_beam_gather_equals_the_reference():
    from kvq import nnops
    V, B, W, L, t = 97, 3, 3, 12, 7
    st, _, _ = BR.select_case(V, 104, B, W, torch.float32, 11, L=L, t=t)
    st["lengths"][:] = np.random.default_rng(1).integers(0, L + 1, st["lengths"].shape[0])
    dev = BR.state_to(st, "cuda")
    ow, out = framed(st["ids"].shape, torch.int64, fill=-3)
    nnops.beam_gather(state(t, Lmax=L, pad=6), dev["ids"], dev["anc"], dev["lengths"], out=out)
    torch.cuda.synchronize()
    assert guards_intact(ow) and np.array_equal(out.cpu().numpy(), BR.gather_ref(st, t, 6))
    nnops.beam_gather(state(L, Lmax=L, pad=6), dev["ids"], dev["anc"], dev["lengths"], out=out.fill_(-3))      # t outside: nothing stored
    torch.cuda.synchronize()
    assert bool((out == -3).all())


# ---------------------------------------------------------------------------------------------------------------- attention
def attn_inputs(R, nh, dtype, seed):
    H = nh * 64
    g = torch.Generator().manual_seed(seed)
    _, qkv = framed((R, 3 * H), dtype, g)
    cw, cache = framed((R, 128, 2 * H), dtype, g)
    return qkv, cw, cache


@pytest.mark.parametrize("dtype,ts", [(torch.bfloat16, (0, 1, 8, 63, 127)), (torch.float32, (31,))])
def test_beam_attn_self_is_gen_attn_on_the_gathered_cache_bit_for_bit(dtype, ts):
    from kvq import nnops
    R, nh, L = 12, 2, 128
    H = nh * 64
    for t in ts:
        qkv, cw, cache = attn_inputs(R, nh, dtype, 40 + t)
        g = torch.Generator().manual_seed(t)
        anc = torch.randint(0, R, (2, R, L), generator=g, dtype=torch.int32)      # a random slot for every (row, position)
        anc[(t & 1) ^ 1] = -77                                                    # the other half is never read (a slot outside reads row r)
        anc[t & 1, :, t + 1:] = 10 ** 6                                           # nor are positions behind t
        aw, anc_dev = framed((2, R, L), torch.int32)
        anc_dev.copy_(anc)
        gathered = cache.clone()                                                  # row (r, j) := row (anc[r, j], j), physically
        idx = anc[t & 1, :, :t + 1].long().cuda()
        gathered[:, :t + 1] = cache[idx, torch.arange(t + 1, device="cuda").unsqueeze(0)]
        st = state(t)
        want = nnops.gen_attn_self(st, qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], gathered, nh)
        before = cw.clone()
        ow, out = framed((R, H + 64), dtype, fill=3.0)
        nnops.beam_attn_self(st, qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], cache, anc_dev, nh, out=out[:, :H])
        torch.cuda.synchronize()
        assert torch.equal(out[:, :H], want), f"t={t}"
        assert bool((out[:, H:] == 3.0).all()) and guards_intact(ow) and guards_intact(aw) and torch.equal(anc_dev.cpu(), anc)
        # the stored row (r, t) is the projection's, and nothing else of the cache changed
        assert torch.equal(cache[:, t, :H], qkv[:, H:2 * H]) and torch.equal(cache[:, t, H:], qkv[:, 2 * H:]), t
        after = cw.clone()
        after[GUARD:-GUARD].view(R, 128, 2 * H)[:, t] = before[GUARD:-GUARD].view(R, 128, 2 * H)[:, t]
        assert torch.equal(after, before), f"t={t}: the cache changed outside row t"
        # and the values pass the judge of kvq_gen_attn
        ref, term = GR.attn_ref(GR.heads(qkv[:, :H], nh), GR.heads(gathered[:, :t + 1, :H], nh), GR.heads(gathered[:, :t + 1, H:], nh))
        ok, worst = GR.attn_judge(GR.heads(out[:, :H], nh), ref, term, dtype)
        assert ok, f"t={t}: worst |got - ref| / bound = {worst:.3f}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_beam_attn_identity_ancestry_and_one_row_per_sentence_is_gen_attn(dtype):
    from kvq import nnops
    R, nh, L, t = 5, 2, 128, 20
    H = nh * 64
    qkv, _, cache = attn_inputs(R, nh, dtype, 5)
    twin = cache.clone()
    anc = torch.arange(R, dtype=torch.int32, device="cuda").view(1, R, 1).expand(2, R, L).contiguous()
    st = state(t)
    want = nnops.gen_attn_self(st, qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], twin, nh)
    got = nnops.beam_attn_self(st, qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], cache, anc, nh)
    assert torch.equal(got, want) and torch.equal(cache, twin)
    kv = cache[:, :12].reshape(R * 12, 2 * H)
    assert torch.equal(nnops.beam_attn_cross(st, qkv[:, :H], kv, 12, nh, 1), nnops.gen_attn_cross(st, qkv[:, :H], kv, 12, nh))
    # a position outside the cache stores nothing
    ow, out = framed((R, H), dtype, fill=3.0)
    small = cache[:, :16].contiguous()
    keep = small.clone()
    nnops.beam_attn_self(state(16), qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], small, anc[:, :, :16].contiguous(), nh, out=out)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all()) and torch.equal(small, keep) and guards_intact(ow)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_beam_attn_cross_reads_the_sentence_of_its_row_bit_for_bit(dtype):
    from kvq import nnops
    from kvq._ffi import KvqError
    S, rps, nh, Se = 4, 3, 2, 12
    R, H = 11, nh * 64                                                 # the last sentence has two rows only
    g = torch.Generator().manual_seed(8)
    pw, proj = framed((S * Se, 3 * 2 * H), dtype, g)                   # three layers' keys | values side by side
    _, q = framed((R, H), dtype, g)
    kv = proj[:, 2 * H:4 * H]
    before = pw.clone()
    ow, out = framed((R, H), dtype, fill=3.0)
    st = state(5)
    nnops.beam_attn_cross(st, q, kv, Se, nh, rps, out=out)
    torch.cuda.synchronize()
    repeated = kv.reshape(S, Se, 2 * H).repeat_interleave(rps, dim=0)[:R].reshape(R * Se, 2 * H).contiguous()
    assert torch.equal(out, nnops.gen_attn_cross(st, q, repeated, Se, nh))
    assert torch.equal(pw, before) and guards_intact(ow)
    kv3 = repeated.reshape(R, Se, 2 * H)
    ref, term = GR.attn_ref(GR.heads(q, nh), GR.heads(kv3[:, :, :H], nh), GR.heads(kv3[:, :, H:], nh))
    assert GR.attn_judge(GR.heads(out, nh), ref, term, dtype)[0]
    with pytest.raises(KvqError):
        nnops.beam_attn_cross(st, q, kv[:3 * Se], Se, nh, rps)            # fewer sentences than ceil(R / rows_per_sentence)


def test_beam_kernels_refuse_what_they_cannot_do():
    from kvq import nnops
    from kvq._ffi import KvqError
    st8 = BR.new_state(1, 8, 4, [[1]], 0)
    dev = BR.state_to(st8, "cuda")
    args = lambda d: (d["ids"], d["parent"], d["scores"], d["step_scores"], d["anc"], d["finished"], d["lengths"])
    x = torch.zeros((8, 8), device="cuda")
    for W in (0, 9, True, 2.0):
        with pytest.raises(KvqError):
            nnops.beam_select(state(0, Lmax=4), x, 8, W, *args(dev))
    with pytest.raises(KvqError):
        nnops.beam_select(state(0, Lmax=4), x, 4, 8, *args(dev))       # more beams than tokens
    with pytest.raises(KvqError):
        nnops.beam_select(state(0, Lmax=4), x, 8, 8, *args(dict(dev, anc=dev["anc"][:, :, :3].contiguous())))
    with pytest.raises(KvqError):
        nnops.beam_select(state(0, Lmax=4), x, 8, 8, *args(dict(dev, scores=dev["scores"].double())))
