"""kvq_attn_probs against f64: the per-sentence probabilities, the f64 table of their sum over sentences, accumulation, determinism.

Reference: masked_softmax(q k^T scale, attend_allowed(...), empty_rows_zero=True) in f64 on the upcast inputs (tests/_dropout_ref.py).

Bound on the per-sentence P:  |got - ref| <= 2 (2^-14 ref + 2^-24).  From tests/_attn_ref.py's constants: the scores carry about
2^-16 of error (f32 accumulation of 64 products, the scale, the exponent's argument reduction) and LSE_ATOL = 2^-15 bounds what
the exponent as a whole is off by; exp() turns an absolute error of the exponent into a relative one of P, 2^-15 + 2^-16 < 2^-14.
2^-24 is half an ulp of 1, for the probabilities near 0; the factor 2 is margin, as elsewhere in that file.  Row sums: within 2^-20
of 1 (32 .. 128 f32 roundings of 2^-24 that do not line up).  Worst ratio |got - ref| / (2^-14 ref + 2^-24) per case, which the
bound asks to stay <= 2, and worst |row sum - 1|, as measured on an MI355X:
    case                      ratio    |row sum - 1|        case                      ratio    |row sum - 1|
    mfma_qkv_5x3x32x32        0.0080   1.7e-07              f32_4x2x12x12_causal      0.0098   1.5e-07
    mfma_4x2x12x12            0.0064   1.2e-07              f32_4x2x7x19              0.0101   1.6e-07
    mfma_cross_4x2x7x19       0.0083   1.3e-07              blk_3x2x33x33_causal      0.0086   1.3e-07
    mfma_3x2x1x1              0        0                    blk_2x2x40x128            0.0104   2.3e-07
    mfma_empty_2x2x32x32      0.0066   1.3e-07              blk_2x2x128x128           0.0103   3.0e-07
    mfma_runs_301x12x12x12    0.0118   1.8e-07              blk_empty_2x2x40x40       0.0088   1.8e-07
The derived bound is not wrong, it is loose by two orders of magnitude: at these shapes (scores of a few units) the exponent is off
by about 2^-21, not 2^-15 -- LSE_ATOL covers the forward's log of the row sum as well, which the probabilities never go through.
(every case prints its two figures before it asserts: pytest -s).
"""
import functools
import zlib

import pytest
import torch

from _dropout_ref import attend_allowed, masked_softmax

BF16, F32 = torch.bfloat16, torch.float32
P_REL, P_ABS, MARGIN = 2.0 ** -14, 2.0 ** -24, 2.0
ROWSUM_TOL = 2.0 ** -20
TABLE_RTOL = 1e-12

# B x nh x Sq x Sk.  layout "qkv": the engine's fused [N, 3H] self-attention buffer; "cross": k | v the halves of one [B*Sk, 2H].
# runs of sentences per workgroup: max(8, ceil(B nh / 1024)) -- B <= 8: one run; B = 301, nh = 12: 37 runs of 8 and one of 5.
CASES = {
    "mfma_qkv_5x3x32x32": dict(B=5, nh=3, Sq=32, Sk=32, dt=BF16, causal=True, mask="ragged", layout="qkv"),
    "mfma_4x2x12x12": dict(B=4, nh=2, Sq=12, Sk=12, dt=BF16, causal=False, mask="ragged", layout="qkv"),
    "mfma_cross_4x2x7x19": dict(B=4, nh=2, Sq=7, Sk=19, dt=BF16, causal=False, mask=None, layout="cross"),
    "mfma_3x2x1x1": dict(B=3, nh=2, Sq=1, Sk=1, dt=BF16, causal=False, mask=None, layout="qkv"),
    "mfma_empty_2x2x32x32": dict(B=2, nh=2, Sq=32, Sk=32, dt=BF16, causal=False, mask="empty1", layout="qkv"),
    "mfma_runs_301x12x12x12": dict(B=301, nh=12, Sq=12, Sk=12, dt=BF16, causal=True, mask="ragged", layout="qkv"),
    "f32_4x2x12x12_causal": dict(B=4, nh=2, Sq=12, Sk=12, dt=F32, causal=True, mask="ragged", layout="qkv"),
    "f32_4x2x7x19": dict(B=4, nh=2, Sq=7, Sk=19, dt=F32, causal=False, mask=None, layout="cross"),
    "blk_3x2x33x33_causal": dict(B=3, nh=2, Sq=33, Sk=33, dt=BF16, causal=True, mask="ragged", layout="qkv"),
    "blk_2x2x40x128": dict(B=2, nh=2, Sq=40, Sk=128, dt=BF16, causal=False, mask=None, layout="cross"),
    "blk_2x2x128x128": dict(B=2, nh=2, Sq=128, Sk=128, dt=BF16, causal=False, mask="ragged", layout="qkv"),
    "blk_empty_2x2x40x40": dict(B=2, nh=2, Sq=40, Sk=40, dt=BF16, causal=False, mask="empty1", layout="qkv"),
}


def make_inputs(name):
    """CPU tensors of the case: q [B*Sq, H], k, v [B*Sk, H] in the io dtype, mask [B, Sk] int64 or None"""
    c = CASES[name]
    B, nh, Sq, Sk = c["B"], c["nh"], c["Sq"], c["Sk"]
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    H = nh * 64
    q = torch.randn(B * Sq, H, generator=gen).to(c["dt"])
    k = torch.randn(B * Sk, H, generator=gen).to(c["dt"])
    v = torch.randn(B * Sk, H, generator=gen).to(c["dt"])
    mask = None
    if c["mask"] is not None:
        lens = torch.randint(1, Sk + 1, (B,), generator=gen)
        lens[0] = Sk
        lens[-1] = max(1, Sk // 3)
        mask = (torch.arange(Sk)[None] < lens[:, None]).long()
        if c["mask"].startswith("empty"):
            mask[int(c["mask"][5:])] = 0
    return q, k, v, mask


def heads(t, B, S, nh):
    return t.reshape(B, S, nh, 64).permute(0, 2, 1, 3)


def reference(name, q, k, mask, causal=None, mask_edit=None, tril_diagonal=0, swap_heads=None):
    """f64 probabilities [B, nh, Sq, Sk] and the attend pattern; the three keyword edits are the sensitivity test's mutations"""
    c = CASES[name]
    B, nh, Sq, Sk = c["B"], c["nh"], c["Sq"], c["Sk"]
    s = heads(q.double(), B, Sq, nh) @ heads(k.double(), B, Sk, nh).transpose(-1, -2) * 0.125
    m = mask if mask_edit is None else mask_edit(mask.clone())
    allow = attend_allowed(B, Sq, Sk, m, False, "cpu")
    if c["causal"] if causal is None else causal:
        allow = allow & torch.ones(Sq, Sk, dtype=torch.bool).tril(tril_diagonal)[None, None]
    p = masked_softmax(s, allow, empty_rows_zero=True)
    if swap_heads is not None:
        p = p.clone()
        p[:, list(swap_heads)] = p[:, list(reversed(swap_heads))]
    return p, allow.expand(B, nh, Sq, Sk)


def worst_ratio(got, ref):
    return float(((got.double() - ref).abs() / (P_REL * ref + P_ABS)).max())


GUARD = 64


def _guarded(n, dtype, fill):
    flat = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return flat, flat[GUARD:GUARD + n]


def _launch(name, dev_in):
    """one fresh call: (probs, table, guards_ok)"""
    from kvq import nnops
    c = CASES[name]
    B, nh, Sq, Sk = c["B"], c["nh"], c["Sq"], c["Sk"]
    q, k, v, mask, lse = dev_in
    pf, pv = _guarded(B * nh * Sq * Sk, torch.float32, float("nan"))
    tf, tv = _guarded(nh * Sq * Sk, torch.float64, 0.0)
    tf[:GUARD] = 7.0
    tf[-GUARD:] = 7.0
    probs, table = pv.view(B, nh, Sq, Sk), tv.view(nh, Sq, Sk)
    nnops.attn_probs(q, k, v, mask, B, nh, Sq, Sk, c["causal"], lse=lse, probs=probs, table=table)
    return probs, table, (pf, tf)


def _guards_ok(pf, tf):
    return bool(torch.isnan(pf[:GUARD]).all() and torch.isnan(pf[-GUARD:]).all() and (tf[:GUARD] == 7.0).all() and (tf[-GUARD:] == 7.0).all())


@functools.lru_cache(maxsize=None)
def run_case(name):
    """Everything the assertions need, computed once: two fresh launches, a third call on top of the first one's table, and the f64
    reference.  Host tensors."""
    from kvq import nnops
    c = CASES[name]
    B, nh, Sq, Sk = c["B"], c["nh"], c["Sq"], c["Sk"]
    H = nh * 64
    q, k, v, mask = make_inputs(name)
    ref, allow = reference(name, q, k, mask)
    if c["layout"] == "qkv":                               # one [N, 3H] buffer, as BertSelfAttention's fused projection leaves it
        X = torch.cat([q, k, v], 1).cuda()
        dq, dk, dv = X[:, :H], X[:, H:2 * H], X[:, 2 * H:]
    else:                                                  # cross-attention: q alone, k | v the halves of the encoder-side buffer
        dq = q.cuda()
        KV = torch.cat([k, v], 1).cuda()
        dk, dv = KV[:, :H], KV[:, H:]
    dmask = mask.cuda() if mask is not None else None
    lse = None
    if max(Sq, Sk) > 32:
        _, lse = nnops.attn_fwd(dq, dk, dv, dmask, B, nh, Sq, Sk, c["causal"])
    dev_in = (dq, dk, dv, dmask, lse)
    p1, t1, g1 = _launch(name, dev_in)
    t_once = t1.clone()
    nnops.attn_probs(dq, dk, dv, dmask, B, nh, Sq, Sk, c["causal"], lse=lse, table=t1)      # table only, on top of the first call
    p2, t2, g2 = _launch(name, dev_in)
    torch.cuda.synchronize()
    return dict(ref=ref, allow=allow, probs=p1.cpu(), table=t_once.cpu(), table_twice=t1.cpu(), probs_again=p2.cpu(), table_again=t2.cpu(),
                guards=_guards_ok(*g1) and _guards_ok(*g2))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_probabilities_table_accumulation_and_determinism(name):
    r = run_case(name)
    got, ref, allow = r["probs"], r["ref"], r["allow"]
    ratio = worst_ratio(got, ref)
    some = allow.any(-1)
    rowsum = got.double().sum(-1)
    worst_sum = float((rowsum[some] - 1).abs().max()) if bool(some.any()) else 0.0
    print(f"\n[attn_probs] {name}: worst |got - ref| / (2^-14 ref + 2^-24) = {ratio:.4f} (bound {MARGIN}), "
          f"worst |row sum - 1| = {worst_sum:.3e} (bound {ROWSUM_TOL:.3e})")
    assert r["guards"], "written outside probs / table"
    assert not bool(torch.isnan(got).any()), "NaN (or an element that was never written) in the probabilities"
    # per-sentence P
    assert ratio <= MARGIN, f"{name}: worst ratio {ratio}"
    # probability rows
    assert worst_sum <= ROWSUM_TOL
    assert bool((got[~allow] == 0).all()), "a masked / non-causal position is not exactly 0"
    assert bool((rowsum[~some] == 0).all()), "a query row without attended keys is not all-zero"
    # table = the f64 sum over sentences of the kernel's own P
    own = got.double().sum(0)
    assert bool(((r["table"] - own).abs() <= TABLE_RTOL * own.abs()).all()), float((r["table"] - own).abs().max())
    # accumulation: the same sum added once more
    assert torch.equal(r["table_twice"], 2 * r["table"])
    # determinism: a fresh run, the same bits
    assert torch.equal(r["probs_again"].view(torch.int32), got.view(torch.int32))
    assert torch.equal(r["table_again"].view(torch.int64), r["table"].view(torch.int64))


def test_the_bound_sees_a_dropped_key_a_shifted_causal_edge_and_swapped_heads():
    """CPU: the f64 reference of the 32 x 32 case with one defect each, judged against the clean one as the kernel's output would
    be -- each must break the P bound, or the bound shows nothing."""
    name = "mfma_qkv_5x3x32x32"
    q, k, v, mask = make_inputs(name)
    ref, _ = reference(name, q, k, mask)

    def drop_last_attended(m):
        last = m.sum(1) - 1                                # prefix masks: the last attended key of sentence b
        m[torch.arange(m.shape[0]), last] = 0
        return m
    mutants = {
        "last attended key dropped": reference(name, q, k, mask, mask_edit=drop_last_attended)[0],
        "causal edge off by one": reference(name, q, k, mask, tril_diagonal=1)[0],
        "heads 0 and 2 swapped": reference(name, q, k, mask, swap_heads=(0, 2))[0],
    }
    assert worst_ratio(ref.float(), ref) <= MARGIN         # (the clean reference rounded to f32 passes)
    for what, mut in mutants.items():
        ratio = worst_ratio(mut.float(), ref)
        print(f"[attn_probs] {what}: ratio {ratio:.1f}")
        assert ratio > MARGIN, what


@pytest.mark.gpu
def test_entry_point_captures_as_two_kernel_nodes_and_replays_the_eager_bits():
    """include/kvq.h: kernels only -- no memset / memcpy node in a captured call (slabs in the caller's workspace)."""
    import ctypes
    from kvq import nnops
    from kvq._ffi import check, lib
    name = "mfma_qkv_5x3x32x32"
    c = CASES[name]
    B, nh, Sq, Sk, H = c["B"], c["nh"], c["Sq"], c["Sk"], c["nh"] * 64
    q, k, v, mask = make_inputs(name)
    X = torch.cat([q, k, v], 1).cuda()
    dq, dk, dv, dmask = X[:, :H], X[:, H:2 * H], X[:, 2 * H:], mask.cuda()
    probs = torch.empty(B, nh, Sq, Sk, device="cuda")
    table = torch.zeros(nh, Sq, Sk, dtype=torch.float64, device="cuda")
    nnops.attn_probs(dq, dk, dv, dmask, B, nh, Sq, Sk, True, probs=probs, table=table)      # eager (and the workspace exists from here on)
    want_p, want_t = probs.clone(), table.clone()
    table.zero_()
    probs.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g.capture_begin()
        nnops.attn_probs(dq, dk, dv, dmask, B, nh, Sq, Sk, True, probs=probs, table=table)
        g.capture_end()
    torch.cuda.current_stream().wait_stream(s)
    counts = (ctypes.c_int64 * 6)()
    check(lib().kvq_graph_census(g.raw_cuda_graph(), counts), "kvq_graph_census")
    kinds = dict(zip(("kernel", "memset", "memcpy", "empty", "event", "other"), counts))
    assert kinds["kernel"] == 2 and kinds["memset"] == 0 and kinds["memcpy"] == 0 and kinds["other"] == 0, kinds
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(probs, want_p) and torch.equal(table, want_t)


@pytest.mark.gpu
def test_refusals_return_the_error_status_and_do_not_fault():
    from kvq import _ffi, nnops
    from kvq._ffi import KvqError
    lib = _ffi.lib()
    H = 2 * 64

    def bufs(B, Sq, Sk, dt=BF16):
        g = torch.Generator().manual_seed(5)
        return (torch.randn(B * Sq, H, generator=g).to(dt).cuda(), torch.randn(B * Sk, H, generator=g).to(dt).cuda(),
                torch.randn(B * Sk, H, generator=g).to(dt).cuda())
    # the blocked path without the forward's lse
    q, k, v = bufs(2, 33, 33)
    probs = torch.zeros(2, 2, 33, 33, device="cuda")
    with pytest.raises(KvqError, match="log-sum-exp"):
        nnops.attn_probs(q, k, v, None, 2, 2, 33, 33, False, probs=probs)
    # above 32 tokens in f32
    qf, kf, vf = bufs(2, 33, 33, F32)
    with pytest.raises(KvqError, match="bf16 only"):
        nnops.attn_probs(qf, kf, vf, None, 2, 2, 33, 33, False, probs=probs)
    # above 128 tokens
    q2, k2, v2 = bufs(1, 129, 129)
    big = torch.zeros(1, 2, 129, 129, device="cuda")
    with pytest.raises(KvqError, match="128-token"):
        nnops.attn_probs(q2, k2, v2, None, 1, 2, 129, 129, False, lse=torch.zeros(1, 2, 129, device="cuda"), probs=big)
    # head dim != 64 (the wrapper always passes 64: straight to the C ABI)
    q3, k3, v3 = bufs(2, 12, 12)
    p3 = torch.zeros(2, 4, 12, 12, device="cuda")
    rc = lib.kvq_attn_probs(q3.data_ptr(), k3.data_ptr(), v3.data_ptr(), None, None, 2, 4, 12, 12, 32, H, H, H, 0, 0.125, _ffi.KVQ_BF16,
                            p3.data_ptr(), None, None, 0, _ffi.stream_ptr())
    assert rc == -1 and b"head dim 32" in lib.kvq_last_error()
    # neither output; a table without its workspace
    with pytest.raises(KvqError, match="neither"):
        nnops.attn_probs(q3, k3, v3, None, 2, 2, 12, 12, False)
    rc = lib.kvq_attn_probs(q3.data_ptr(), k3.data_ptr(), v3.data_ptr(), None, None, 2, 2, 12, 12, 64, H, H, H, 0, 0.125, _ffi.KVQ_BF16,
                            None, torch.zeros(2, 12, 12, dtype=torch.float64, device="cuda").data_ptr(), None, 0, _ffi.stream_ptr())
    assert rc == -1 and b"workspace" in lib.kvq_last_error()
    torch.cuda.synchronize()                               # nothing was launched, nothing faulted
    assert bool((probs == 0).all()) and bool((big == 0).all()) and bool((p3 == 0).all())
    # and the device still serves a valid call
    ok = torch.empty(2, 2, 12, 12, device="cuda")
    nnops.attn_probs(q3, k3, v3, None, 2, 2, 12, 12, False, probs=ok)
    assert float((ok.sum(-1) - 1).abs().max()) <= ROWSUM_TOL
