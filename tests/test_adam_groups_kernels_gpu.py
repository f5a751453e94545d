"""Per-element parity of kvq_adam_step_grouped / _grouped_guarded (adam_group_kernel) and of kvq_step_state_advance_sched
(csrc/kvq_adam.hip) against f64: the judges of tests/_adam_groups_ref.py (counted f32 roundings; tests/test_adam_groups_ref.py checks
them on the CPU), the frames, states and tallies of tests/test_adam_parity_gpu.py."""
import pytest
import torch

import _adam_groups_ref as G
import _adam_ref as R
from test_adam_parity_gpu import BF16, F32, JUDGE_SLICE, Tally, big_inputs, frame_intact, framed, guard_with, state_at

pytestmark = pytest.mark.gpu

POISON = 0xE0                                                  # high nibble of the table entries no launch may read (poison())
ALL_SCALES, ALL_DECAYS = (0.0, 0.1, 1.0, 10.0), (0.0, 0.01)
TABLES = {2: ([0.1, 10.0], [0.01, 0.0]),
          16: ([ALL_SCALES[j % 4] for j in range(16)], [ALL_DECAYS[(j // 4) % 2] for j in range(16)])}
NS = (16, 32, 48 + 4 + 3, 2048 + 4 + 3)
FIRSTS = (0, 16, 4096 + 16)


@pytest.fixture(scope="module")
def ops():
    from kvq import _ffi, nnops
    _ffi.lib()
    assert torch.cuda.is_available()
    return nnops


def poison(n_groups, first_group, last_group):
    """An out-of-range id for the entries outside a launch.  The kernel masks an id to its low nibble, so what a stray read of such an
    entry would use is LDS entry `id & 15`: with fewer than 16 groups entry 15, which the kernel zeroes (lr 0, wd 0: unlike every
    group of TABLES[2]); with 16 groups every entry is a real group, and the nibble is one whose lr_scale differs from the scale of
    the launch's first and last block -- the two blocks beside the poisoned entries."""
    if n_groups < 16:
        return POISON | 15
    scale = TABLES[16][0]
    return POISON | next(j for j in range(16) if scale[j] not in (scale[first_group], scale[last_group]))


def block_table(n, first, n_groups, run=1):
    """uint8 CPU table of a flat buffer that holds the launch [first, first + n): the launch's blocks cycle through the groups, a new
    one every `run` blocks; every other entry is poisoned (poison())."""
    lo, hi = first // 16, (first + n + 15) // 16
    own = ((torch.arange(hi - lo) // run) % n_groups).to(torch.uint8)
    blocks = torch.full((hi + 8,), poison(n_groups, int(own[0]), int(own[-1])), dtype=torch.uint8)
    blocks[lo:hi] = own
    assert int(blocks.max()) >= 16 and all(int(b) >= 16 for b in blocks[hi:]) and all(int(b) >= 16 for b in blocks[:lo])
    return blocks


def launch(ops, x, c, st, blocks, first, scale, wd, decoupled, coef=None, skip=0, n_groups=None):
    """One grouped launch of case c on inputs x (CPU), every buffer a view inside a frame of sentinels.  Returns (out on the CPU,
    frames intact)."""
    frames = {k: framed(x[k]) for k in ("p", "m", "v", "vmax") if x[k] is not None}
    frames["shadow"] = framed(n=c.n, dtype=BF16)
    gw, g = framed(x["g"])
    view = lambda k: frames[k][1] if k in frames else None
    dev = lambda t, dt: torch.tensor(t, dtype=dt, device="cuda") if t is not None else None
    ops.adam_step_grouped(view("p"), g, view("m"), view("v"), st, beta1=c.betas[0], beta2=c.betas[1], eps=R.ADAM_EPS, weight_decay=c.wd,
                          vmax=view("vmax"), shadow=view("shadow"), grad_scale=c.grad_scale,
                          guard=guard_with(ops, coef if coef is not None else 1.0, skip) if (coef is not None or skip) else None,
                          block_group=blocks.cuda() if blocks is not None else None, first_element=first,
                          group_lr_scale=dev(scale, F32), group_wd=dev(wd, F32),
                          n_groups=n_groups or (len(scale) if scale is not None else 1), decoupled=decoupled)
    torch.cuda.synchronize()
    intact = all(frame_intact(w) for w, _ in frames.values()) and frame_intact(gw) and torch.equal(g.cpu(), x["g"])
    return {k: (view(k).cpu() if k in frames else None) for k in ("p", "m", "v", "vmax", "shadow")}, intact


def launches():
    """Every n with every first element; gradient dtype, amsgrad, table size, grad_scale, betas and t cycle at different strides, so
    that each value of each meets each n."""
    out = []
    for i, (n, first) in enumerate((n, f) for n in NS for f in FIRSTS):
        c = R.Case(n=n, gdtype=(F32, BF16)[i % 2], amsgrad=bool((i // 2) % 2), wd=0.3, grad_scale=(1.0, 1.0 / 3.0, 1024.0)[i % 3],
                   betas=((0.9, 0.999), (0.5, 0.9999))[(i // 3) % 2], t=(1, 2, 5, 1000)[i % 4], seed=500 + i)
        out.append((c, first, (16, 2)[(i + i // 3) % 2]))
    return out


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
@pytest.mark.parametrize("coef", [None, 0.37], ids=["dev", "guarded-0.37"])
def test_grouped_parity(ops, coef, decoupled):
    """A table that changes group at every block, 2 and 16 groups holding every lr_scale of {0, 0.1, 1, 10} and wd of {0, 0.01}, at
    first elements 0, 16 and 4112 of a table poisoned everywhere else; c.wd = 0.3 would show wherever a group's own decay is not used."""
    tally, seen = Tally(), set()
    for c, first, ng in launches():
        scale, wd = TABLES[ng]
        x, blocks = R.case_inputs(c), block_table(c.n, first, ng)
        st = state_at(ops, c.t, R.LR, *c.betas)
        out, intact = launch(ops, x, c, st, blocks, first, scale, wd, decoupled, coef)
        what = f"n = {c.n}, first {first}, {ng} groups, g {str(c.gdtype)[6:]}, amsgrad {c.amsgrad}, t = {c.t}"
        assert intact, f"{what}: a sentinel around a buffer changed"
        assert torch.equal(R.bf16_bits(out["shadow"]), R.bf16_rne_bits(out["p"])), f"{what}: shadow is not bf16(p')"
        grp = G.element_groups(blocks, first, c.n)
        s_e, wd_e = G.element_tables(grp, scale, wd)
        ratios = G.grouped_ratios(out, x, R.case_hyper(c, coef), s_e, wd_e, decoupled)
        if not c.amsgrad:
            ratios.pop("vmax", None)
        tally.add(ratios, c.n, what)
        seen |= {(c.n, first), (c.n, c.gdtype), (c.n, c.amsgrad), (c.n, ng)}
        zero = s_e == 0                                                    # lr_scale 0 is not frozen: the moments move, p keeps its
        if bool(zero.any()) and not decoupled:                             # bits (coupled: u = 0 and no decay factor)
            assert torch.equal(out["p"][zero], x["p"][zero]) and not torch.equal(out["m"][zero], x["m"][zero])
    assert seen >= {(n, v) for n in NS for v in FIRSTS + (F32, BF16, False, True, 2, 16)}
    w = tally.report(f"grouped coef {coef} decoupled {decoupled}")
    assert tally.paths >= {"8-chunk", "odd 4-chunk", "scalar tail"}
    assert w <= 1.0, tally.worst


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_one_group_form(ops, decoupled):
    """block_group = NULL: entry 0 of both tables for the whole launch (the aux parameters, a range inside one group)."""
    tally = Tally()
    for i, n in enumerate(NS):
        c = R.Case(n=n, gdtype=(F32, BF16)[i % 2], amsgrad=bool(i % 2), wd=0.3, grad_scale=1.0 / 3.0, betas=(0.9, 0.999), t=3, seed=600 + i)
        x = R.case_inputs(c)
        out, intact = launch(ops, x, c, state_at(ops, c.t, R.LR, *c.betas), None, 0, [10.0], [0.01], decoupled)
        assert intact
        s_e, wd_e = torch.full((n,), 10.0, dtype=torch.float64), torch.full((n,), float(R.f32(0.01)), dtype=torch.float64)
        ratios = G.grouped_ratios(out, x, R.case_hyper(c), s_e, wd_e, decoupled)
        if not c.amsgrad:
            ratios.pop("vmax", None)
        tally.add(ratios, n, f"one group, n = {n}")
    assert tally.report(f"one group decoupled {decoupled}") <= 1.0, tally.worst


@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_skip_stores_nothing(ops, decoupled):
    """guard->skip = 1: p, m, v, vmax and the shadow keep their bits, the frames theirs."""
    for n, first in ((2048 + 4 + 3, 16), (16, 0)):
        c = R.Case(n=n, gdtype=BF16, amsgrad=True, wd=0.01, grad_scale=1.0, betas=(0.9, 0.999), t=2, seed=700)
        x = R.case_inputs(c)
        out, intact = launch(ops, x, c, state_at(ops, c.t, R.LR, *c.betas), block_table(n, first, 16), first, *TABLES[16], decoupled,
                             coef=0.37, skip=1)
        assert intact
        for k in ("p", "m", "v", "vmax"):
            assert torch.equal(out[k].view(torch.int32), x[k].view(torch.int32)), f"a skipped launch changed {k}"
        assert bool((out["shadow"] == 77.0).all()), "a skipped launch wrote the shadow"


@pytest.mark.parametrize("guarded", [False, True], ids=["dev", "guarded"])
def test_default_groups_give_the_bits_of_adam_step_dev(ops, guarded):
    """Every scale 1, every decay the launch's, decoupled 0: the bits of kvq_adam_step_dev / _guarded on covering_cases' inputs --
    through a table, through NULL tables and through the one-group form."""
    coef = 0.37 if guarded else None
    for c in R.covering_cases():
        x = R.case_inputs(c)
        st = state_at(ops, c.t, R.LR, *c.betas)
        fr = {k: framed(x[k]) for k in ("p", "m", "v", "vmax", "g") if x[k] is not None}
        fr["shadow"] = framed(n=c.n, dtype=BF16)
        v = lambda k: fr[k][1] if k in fr else None
        ops.adam_step_dev(v("p"), v("g"), v("m"), v("v"), st, beta1=c.betas[0], beta2=c.betas[1], eps=R.ADAM_EPS, weight_decay=c.wd,
                          vmax=v("vmax"), shadow=v("shadow"), grad_scale=c.grad_scale, guard=guard_with(ops, coef) if guarded else None)
        torch.cuda.synchronize()
        want = {k: v(k).cpu() for k in ("p", "m", "v", "vmax", "shadow") if v(k) is not None}
        for form, (blocks, scale, wd, ng) in dict(table=(block_table(c.n, 16, 3), [1.0] * 3, [c.wd] * 3, 3),
                                                  null_tables=(block_table(c.n, 16, 3), None, None, 3),
                                                  null_tables_16=(block_table(c.n, 16, 16), None, None, 16),
                                                  null_scale_16=(block_table(c.n, 16, 16), None, [c.wd] * 16, 16),
                                                  one_group=(None, [1.0], [c.wd], 1)).items():
            out, intact = launch(ops, x, c, st, blocks, 16, scale, wd, False, coef, n_groups=ng)
            assert intact
            for k, t in want.items():
                bits = torch.int16 if k == "shadow" else torch.int32
                assert torch.equal(out[k].view(bits), t.view(bits)), f"{form}: {k} differs from kvq_adam_step_dev ({c})"


def test_grid_stride_grouped(ops):
    """The production launch shape, built as test_grid_stride_dev_amsgrad builds its own: one full trip of the capped grid, 1000 chunks
    of a second trip, the odd 4-chunk and a 3-element tail -- under a table of a few long runs, decoupled, bf16 gradient, amsgrad."""
    n, first = R.ADAM_TRIP + 8 * 1000 + 4 + 3, 16
    c = R.Case(n=n, gdtype=BF16, amsgrad=True, wd=0.3, grad_scale=1.0 / 3.0, betas=(0.9, 0.999), t=5, seed=1100)
    scale, wd = TABLES[16]
    blocks = block_table(n, first, 16, run=(n // 16) // 5)              # six runs: the last covers the second trip and both tails
    frames = big_inputs(n, c.seed, c.gdtype, True)
    frames["shadow"] = framed(n=n, dtype=BF16)
    pre = {k: frames[k][1].clone() for k in ("p", "m", "v", "vmax")}
    st = state_at(ops, c.t, R.LR, *c.betas)
    dev_blocks = blocks.cuda()
    ops.adam_step_grouped(frames["p"][1], frames["g"][1], frames["m"][1], frames["v"][1], st, beta1=c.betas[0], beta2=c.betas[1],
                          eps=R.ADAM_EPS, weight_decay=c.wd, vmax=frames["vmax"][1], shadow=frames["shadow"][1], grad_scale=c.grad_scale,
                          block_group=dev_blocks, first_element=first, group_lr_scale=torch.tensor(scale, device="cuda"),
                          group_wd=torch.tensor(wd, device="cuda"), n_groups=16, decoupled=True)
    torch.cuda.synchronize()
    assert all(frame_intact(w) for w, _ in frames.values()), "a sentinel around a buffer changed"
    codes, hp, tally = R.path_codes(n, device="cuda"), R.case_hyper(c), Tally()
    for s in range(0, n, JUDGE_SLICE):
        e = min(s + JUDGE_SLICE, n)
        x = {k: pre[k][s:e] for k in pre}
        x["g"] = frames["g"][1][s:e]
        out = {k: frames[k][1][s:e] for k in pre}
        assert torch.equal(R.bf16_bits(frames["shadow"][1][s:e]), R.bf16_rne_bits(out["p"])), f"shadow is not bf16(p') in [{s}, {e})"
        s_e, wd_e = G.element_tables(G.element_groups(dev_blocks, first + s, e - s), scale, wd)
        tally.add(G.grouped_ratios(out, x, hp, s_e, wd_e, True), n, "grid-stride grouped", first=s, codes=codes[s:e])
    w = tally.report("grid-stride grouped")
    assert tally.paths == set(R.PATHS) and len(torch.unique(blocks[first // 16:(first + n + 15) // 16])) >= 5
    assert w <= 1.0, tally.worst


# ---------------------------------------------------------------------------------------------------------------
# kvq_step_state_advance_sched
# ---------------------------------------------------------------------------------------------------------------
W, T = 4, 9
LR0, GAMMA_LR = 3e-4, 0.1


def _advance_to(ops, t, milestones, kind, ratio, warmup=W, total=T):
    st = ops.new_step_state("cuda")
    st[0] = t - 1
    ops.step_state_advance_sched(st, LR0, GAMMA_LR, milestones, 0.9, 0.999, warmup_steps=warmup, decay_kind=kind,
                                 total_steps=total if kind else 0, min_ratio=ratio)
    return st


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["none", "linear", "cosine"])
@pytest.mark.parametrize("milestones", [[], [3, 8]], ids=["no-milestones", "milestones"])
def test_sched_step_state_parity(ops, kind, milestones):
    for ratio in (0.1, 0.0):
        for t in (1, W - 1, W, W + 1, T - 1, T, T + 5):
            step, lr, bc1, bc2s = ops.read_step_state(_advance_to(ops, t, milestones, kind, ratio))
            assert step == t
            ref = G.sched_ref(t, LR0, GAMMA_LR, milestones, W, kind, T, ratio)
            r = [G.sched_ratio(lr, ref, LR0)] + R.step_state_ratios((bc1, bc2s), R.step_state_ref(t, LR0, GAMMA_LR, milestones, 0.9, 0.999)[1:])
            print(f"FIGURE sched kind {kind} ratio {ratio} t {t}: lr {lr!r} ref {ref!r} ratios {[round(v, 4) for v in r]}")
            assert max(r) <= 1.0, (kind, ratio, t, lr, ref, r)


@pytest.mark.parametrize("milestones", [[], [3, 8]], ids=["no-milestones", "milestones"])
def test_sched_off_gives_the_raw_words_of_step_state_advance(ops, milestones):
    for t in (1, 2, 3, 4, 9, 10, 1000):
        a = _advance_to(ops, t, milestones, 0, 0.0, warmup=0)
        b = ops.new_step_state("cuda")
        b[0] = t - 1
        ops.step_state_advance(b, LR0, GAMMA_LR, milestones, 0.9, 0.999)
        assert torch.equal(a.cpu(), b.cpu()), f"t = {t}"


def test_bad_arguments_are_refused(ops):
    from kvq._ffi import KvqError
    c = R.Case(n=32, gdtype=F32, amsgrad=False, wd=0.0, grad_scale=1.0, betas=(0.9, 0.999), t=1, seed=1)
    x, st = R.case_inputs(c), state_at(ops, 1, R.LR, 0.9, 0.999)
    with pytest.raises(KvqError):
        launch(ops, x, c, st, block_table(32, 16, 2), 24, *TABLES[2], False)                 # first element not a multiple of 16
    with pytest.raises(KvqError):
        launch(ops, x, c, st, block_table(32, 0, 2)[:1], 0, *TABLES[2], False)               # a table shorter than the launch
    with pytest.raises(KvqError):
        launch(ops, x, c, st, None, 0, [1.0] * 17, [0.0] * 17, False)                        # 17 groups
    with pytest.raises(KvqError):
        ops.step_state_advance_sched(st, LR0, 0.1, [], 0.9, 0.999, warmup_steps=4, decay_kind=1, total_steps=4, min_ratio=0.0)
