"""kvq_seq_compare and kvq_seq_compare_accumulate (csrc/kvq_seqcmp.hip) against the plain Python DP and the numpy scatter-add of
tests/_seqcmp_ref.py.  Integers are compared for equality: nothing here has a tolerance.

The lengths {0, 1, 2, 63, 64, 65, 127, 128} sit on the kernel's seams (a lane owns reference columns l + 1 and l + 65 of one
wavefront); small alphabets make many DP paths tie.  Every buffer is framed by sentinels and rows are wider than their lengths,
with a sentinel behind the last token that must not be read as one.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import _seqcmp_ref as SR
from test_generate_kernels_gpu import framed, guards_intact

pytestmark = pytest.mark.gpu

SEAMS = (0, 1, 2, 63, 64, 65, 127, 128)
SENTINEL = 777_777                         # behind every row's last token; outside every alphabet used


def run_compare(hyp, hyp_len, ref, ref_len, hyp_skip=0, Lmax=128, n_bad=None):
    """one launch on framed device copies -> (out [B, 4] numpy, n_bad int)"""
    from kvq import nnops
    hw, h = framed(hyp.shape, torch.int64)
    rw, r = framed(ref.shape, torch.int64)
    ow, out = framed((hyp.shape[0], 4), torch.int32)
    h.copy_(torch.from_numpy(hyp))
    r.copy_(torch.from_numpy(ref))
    hl = torch.tensor(hyp_len, dtype=torch.int32, device="cuda")
    rl = torch.tensor(ref_len, dtype=torch.int32, device="cuda")
    got, bad = nnops.seq_compare(h, hl, r, rl, hyp_skip=hyp_skip, Lmax=Lmax, out=out, n_bad=n_bad)
    torch.cuda.synchronize()
    assert guards_intact(hw) and guards_intact(rw) and guards_intact(ow)
    assert got.data_ptr() == out.data_ptr()
    return out.cpu().numpy(), int(bad.item())


def rows_of(pairs, skip=0, ld_extra=3):
    """[(h tokens, r tokens)] -> hyp [B, ld], hyp_len (prompt included), ref [B, ld], ref_len; SENTINEL wherever no token lies"""
    B = len(pairs)
    ldh = skip + max(len(h) for h, _ in pairs) + ld_extra
    ldr = max(len(r) for _, r in pairs) + ld_extra
    hyp = np.full((B, ldh), SENTINEL, dtype=np.int64)
    ref = np.full((B, ldr), SENTINEL, dtype=np.int64)
    for b, (h, r) in enumerate(pairs):
        hyp[b, skip:skip + len(h)] = h
        ref[b, :len(r)] = r
    return hyp, [skip + len(h) for h, _ in pairs], ref, [len(r) for _, r in pairs]


def check(pairs, skip=0, ld_extra=3):
    hyp, hl, ref, rl = rows_of(pairs, skip, ld_extra)
    want, bad = SR.seq_compare(hyp, hl, ref, rl, hyp_skip=skip)
    assert bad == 0
    got, n_bad = run_compare(hyp, hl, ref, rl, hyp_skip=skip)
    assert n_bad == 0
    wrong = [(b, got[b].tolist(), want[b].tolist()) for b in range(len(pairs)) if not np.array_equal(got[b], want[b])]
    assert not wrong, wrong[:5]
    return got


@pytest.mark.parametrize("alphabet", [2, 3, 30522])
def test_every_combination_of_seam_lengths(alphabet):
    rng = np.random.default_rng(alphabet)
    pairs = [(rng.integers(0, alphabet, n), rng.integers(0, alphabet, m)) for n, m in itertools.product(SEAMS, SEAMS)]
    got = check(pairs)                                                 # B = 64
    assert [tuple(g[2:]) for g in got] == list(itertools.product(SEAMS, SEAMS))


def test_identical_disjoint_and_shifted_pairs():
    rng = np.random.default_rng(7)
    same, disjoint, shifted = [], [], []
    for n in SEAMS:
        r = rng.integers(0, 3, n)
        same.append((r.copy(), r))
        disjoint.append((rng.integers(10, 20, n), rng.integers(30, 40, n)))
        if n:
            r = rng.integers(0, 30522, n)
            shifted.append((r[1:].copy(), r))                          # the first token dropped: one deletion, every position shifted
    got = check(same)
    assert all(g[0] == 0 and g[1] == g[2] for g in got)
    got = check(disjoint)
    assert all(g[0] == g[2] and g[1] == 0 for g in got)
    got = check(shifted)
    assert all(g[0] == 1 for g in got)
    assert all(g[1] <= 2 for g in got if g[3] > 2)                     # ids below 30 522: a chance hit or two at the most


def test_tokens_are_compared_on_all_64_bits():
    pairs = [([5, 6, 7], [5 + 2 ** 32, 6, 7]), ([5 + 2 ** 32], [5]), ([5 + 2 ** 32, 1], [5 + 2 ** 32, 1]), ([-1, 2], [2 ** 32 - 1, 2])]
    got = check(pairs)
    assert got[:, 0].tolist() == [1, 1, 0, 1] and got[:, 1].tolist() == [2, 0, 2, 1]


@pytest.mark.parametrize("B", [1, 5, 9, 64])
@pytest.mark.parametrize("skip", [0, 1, 4])
def test_batch_sizes_prompt_skip_and_wide_rows(B, skip):
    rng = np.random.default_rng(100 * B + skip)
    pairs = []
    for b in range(B):
        n, m = (int(x) for x in rng.choice(SEAMS + (12, 33, 100), 2))
        r = rng.integers(0, 3, m)
        h = rng.integers(0, 3, n) if b % 3 else np.concatenate([r[:m // 2], rng.integers(0, 3, max(n - m // 2, 0))])[:n]
        pairs.append((h, r))
    check(pairs, skip=skip, ld_extra=1 + (B % 4))


def test_rows_whose_lengths_do_not_fit_are_marked_and_counted():
    rng = np.random.default_rng(3)
    pairs = [(rng.integers(0, 3, 20), rng.integers(0, 3, 24)) for _ in range(6)]
    hyp, hl, ref, rl = rows_of(pairs, skip=4)
    hl[1] = 3                                  # hyp_len < hyp_skip
    rl[4] = 25                                 # ref_len > Lmax = 24
    want, bad = SR.seq_compare(hyp, hl, ref, rl, hyp_skip=4, Lmax=24)
    assert bad == 2 and want[1].tolist() == want[4].tolist() == [-1, 0, 0, 0]
    got, n_bad = run_compare(hyp, hl, ref, rl, hyp_skip=4, Lmax=24)
    assert n_bad == 2 and np.array_equal(got, want)
    # the counter accumulates over calls; a length past its own row is refused the same way (it would be read out of bounds)
    counter = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    hl2, rl2 = list(hl), [24] * 6
    hl2[1], hl2[2] = 24, hyp.shape[1] + 1
    got, n_bad = run_compare(hyp, hl2, ref, rl2, hyp_skip=4, Lmax=128, n_bad=counter)
    want, bad = SR.seq_compare(hyp, hl2, ref, rl2, hyp_skip=4, Lmax=128)
    assert bad == 1 and n_bad == 6 and np.array_equal(got, want) and got[2].tolist() == [-1, 0, 0, 0]


def test_the_launcher_refuses_by_status():
    from kvq import _ffi
    lib = _ffi.lib()
    h = torch.zeros((2, 8), dtype=torch.int64, device="cuda")
    l = torch.full((2,), 8, dtype=torch.int32, device="cuda")
    out = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    good = dict(hyp=h.data_ptr(), ld_hyp=8, skip=0, hl=l.data_ptr(), ref=h.data_ptr(), ld_ref=8, rl=l.data_ptr(), B=2, Lmax=8,
                out=out.data_ptr(), bad=bad.data_ptr())
    call = lambda **kw: lib.kvq_seq_compare(*{**good, **kw}.values(), _ffi.stream_ptr())
    assert call() == 0
    for kw, text in ((dict(Lmax=129), "Lmax"), (dict(Lmax=-1), "Lmax"), (dict(skip=-1), "hyp_skip"), (dict(hyp=None), "null"),
                     (dict(hl=None), "null"), (dict(ref=None), "null"), (dict(rl=None), "null"), (dict(out=None), "null"),
                     (dict(bad=None), "null"), (dict(B=-1), "B >= 0")):
        assert call(**kw) == -1 and text in lib.kvq_last_error().decode(), kw
    per = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    slot = torch.zeros((2, 1), dtype=torch.int32, device="cuda")
    table = torch.zeros((1, 6), dtype=torch.int64, device="cuda")
    good = dict(per=per.data_ptr(), B=2, slot=slot.data_ptr(), C=1, R=1, table=table.data_ptr())
    call = lambda **kw: lib.kvq_seq_compare_accumulate(*{**good, **kw}.values(), _ffi.stream_ptr())
    assert call() == 0
    for kw, text in ((dict(C=17), "C must"), (dict(C=0), "C must"), (dict(R=4097), "R must"), (dict(R=0), "R must"), (dict(per=None), "null"),
                     (dict(slot=None), "null"), (dict(table=None), "null")):
        assert call(**kw) == -1 and text in lib.kvq_last_error().decode(), kw
    torch.cuda.synchronize()
    assert table[0].tolist() == [2, 2, 0, 0, 0, 0]


@functools.lru_cache(maxsize=None)
def per_sentence(B=37):
    rng = np.random.default_rng(11)
    per = np.stack([rng.integers(0, 5, B), rng.integers(0, 12, B), rng.integers(0, 13, B), rng.integers(1, 13, B)], axis=1).astype(np.int32)
    per[rng.random(B) < 0.2] = (-1, 0, 0, 0)
    per.setflags(write=False)
    return per


@pytest.mark.parametrize("C", [1, 10])
@pytest.mark.parametrize("R", [1, 43])
def test_accumulate_against_a_numpy_scatter_add(C, R):
    from kvq import nnops
    per = per_sentence()
    B = len(per)
    assert (per[:, 0] < 0).any() and (per[:, 0] == 0).any()
    rng = np.random.default_rng(10 * C + R)
    slot = rng.integers(-1, R + 1, (B, C)).astype(np.int32)          # -1 and R are among them: skipped
    slot[:, 0] = 0
    assert (slot == -1).any() or C == 1
    assert (slot == R).any() or C == 1
    want = SR.accumulate(per, slot, np.zeros((R, 6), dtype=np.int64))
    tw, table = framed((R, 6), torch.int64, fill=0)
    dper, dslot = torch.from_numpy(per.copy()).cuda(), torch.from_numpy(slot).cuda()
    nnops.seq_compare_accumulate(dper, dslot, table)
    torch.cuda.synchronize()
    once = table.cpu().numpy().copy()
    assert guards_intact(tw) and np.array_equal(once, want)
    nnops.seq_compare_accumulate(dper, dslot, table)                   # a second call adds
    torch.cuda.synchronize()
    assert guards_intact(tw) and np.array_equal(table.cpu().numpy(), 2 * want)
    again = torch.zeros((R, 6), dtype=torch.int64, device="cuda")      # the same inputs, the same bits
    nnops.seq_compare_accumulate(dper, dslot, again)
    assert np.array_equal(again.cpu().numpy(), once)
