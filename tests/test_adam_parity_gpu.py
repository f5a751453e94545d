"""Per-element parity of the Adam family (adam_kernel behind kvq_adam_step, _dev, _dev_fp8, _guarded, _guarded_fp8) and of
kvq_step_state_advance (csrc/kvq_adam.hip) against f64.

One step from a random non-zero pre-state, every stored m', v', vmax', p' judged per element inside bounds that count f32
roundings (tests/_adam_ref.py; tests/test_adam_ref.py checks the judges on the CPU); the bf16 shadow bitwise RNE of the stored
p', on chosen ties as well; the fp8 mirror bytewise; every buffer a view inside a frame of sentinels; the grid-stride loop at
the smallest sizes above adam_launch's block cap.  Measured figures: profiles/adam_parity.md."""
import ctypes
import math

import pytest
import torch

import _adam_ref as R

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
PAD = 64                                  # elements of sentinel on either side: 64 bytes for the fp8 mirror, more for the others
SENTINEL = {torch.float32: 77.0, torch.bfloat16: 77.0, torch.uint8: 0xAB, torch.int64: 0x5A5A5A5A5A5A5A5A}
ENTRIES = [("host", None), ("dev", None), ("guarded", 1.0), ("guarded", 0.37)]
CASES = R.covering_cases()


@pytest.fixture(scope="module")
def ops():
    from kvq import _ffi, nnops
    _ffi.lib()
    assert torch.cuda.is_available()
    return nnops


def framed(t=None, n=None, dtype=None):
    """(whole, view): `view` holds t (or n elements of the sentinel) 16-byte aligned inside `whole`, PAD sentinels on both sides."""
    n = t.numel() if t is not None else n
    dtype = t.dtype if t is not None else dtype
    whole = torch.full((n + 2 * PAD,), SENTINEL[dtype], dtype=dtype, device="cuda")
    view = whole[PAD:PAD + n]
    if t is not None:
        view.copy_(t)
    assert view.data_ptr() % 16 == 0
    return whole, view


def frame_intact(whole):
    s = SENTINEL[whole.dtype]
    return bool((whole[:PAD] == s).all()) and bool((whole[-PAD:] == s).all())


def guard_with(ops, coef=1.0, skip=0):
    """A guard state as kvq_grad_guard_finalize leaves it, written from the host."""
    guard = ops.new_grad_guard("cuda")
    guard[1:2].view(torch.float32)[1] = coef
    guard[2] = skip
    return guard


def state_at(ops, t, lr0, b1, b2):
    """A device step state at step t: the count t - 1 written, then advanced once."""
    st = ops.new_step_state("cuda")
    st[0] = t - 1
    ops.step_state_advance(st, lr0, 0.1, [], b1, b2)
    assert ops.read_step_state(st)[0] == t
    return st


def run_entry(ops, entry, coef, c, x, lr=R.LR):
    """One launch of case c on inputs x (CPU) through `entry`.  Returns (out on the CPU: p, m, v, vmax, shadow; frames intact)."""
    frames = {k: framed(x[k]) for k in ("p", "m", "v", "vmax") if x[k] is not None}
    frames["shadow"] = framed(n=c.n, dtype=BF16)
    gw, g = framed(x["g"])
    view = lambda k: frames[k][1] if k in frames else None
    b1, b2 = c.betas
    kw = dict(beta1=b1, beta2=b2, eps=R.ADAM_EPS, weight_decay=c.wd, vmax=view("vmax"), shadow=view("shadow"), grad_scale=c.grad_scale)
    if entry == "host":
        ops.adam_step(view("p"), g, view("m"), view("v"), c.t, lr, **kw)
    else:
        st = state_at(ops, c.t, lr, b1, b2)
        ops.adam_step_dev(view("p"), g, view("m"), view("v"), st, guard=guard_with(ops, coef) if entry == "guarded" else None, **kw)
    torch.cuda.synchronize()
    intact = all(frame_intact(w) for w, _ in frames.values()) and frame_intact(gw) and torch.equal(g.cpu(), x["g"])
    out = {k: (view(k).cpu() if k in frames else None) for k in ("p", "m", "v", "vmax", "shadow")}
    return out, intact


class Tally:
    """Worst ratio per judged output with the element it belongs to, and which code paths were judged."""

    def __init__(self):
        self.worst, self.by_path = {}, {}

    @property
    def paths(self):
        return set(self.by_path)

    def add(self, ratios, n, what, first=0, codes=None):
        for k, r in ratios.items():
            w, where = R.worst(r, n, first)
            if w > self.worst.get(k, (-1.0, ""))[0]:
                self.worst[k] = (w, f"{where}, {what}")
        codes = R.path_codes(n) if codes is None else codes
        for c in torch.unique(codes).tolist():
            w = max(float(r[codes == c].max()) for r in ratios.values())
            self.by_path[R.PATHS[c]] = max(w, self.by_path.get(R.PATHS[c], 0.0))

    def report(self, name):
        for k, (w, where) in sorted(self.worst.items()):
            print(f"FIGURE {name} {k}': worst ratio {w:.4f} at {where}")
        print(f"FIGURE {name} worst ratio per path: " + ", ".join(f"{p} {w:.4f}" for p, w in sorted(self.by_path.items())))
        return max(w for w, _ in self.worst.values())


def case_name(c):
    return (f"n = {c.n}, g {str(c.gdtype)[6:]}, amsgrad {c.amsgrad}, wd {c.wd}, grad_scale {c.grad_scale:.4g}, betas {c.betas}, "
            f"t = {c.t}")


@pytest.mark.parametrize("entry,coef", ENTRIES, ids=["host", "dev", "guarded-1", "guarded-0.37"])
def test_one_step_parity(ops, entry, coef):
    """The covering set of launches (tests/_adam_ref.py: covering_cases) and the two (beta2, t = 2) at which an f32 bias
    correction is visibly off, through one entry point."""
    R.assert_covering(CASES)
    tally, arms = Tally(), [0, 0]
    for c in CASES + R.BC_CASES:
        x = R.case_inputs(c)
        out, intact = run_entry(ops, entry, coef, c, x)
        assert intact, f"{entry}, {case_name(c)}: a sentinel around a buffer changed"
        assert torch.equal(R.bf16_bits(out["shadow"]), R.bf16_rne_bits(out["p"])), f"{entry}, {case_name(c)}: shadow is not bf16(p')"
        ratios = R.launch_ratios(out, x, R.case_hyper(c, coef))
        if c in R.BC_CASES:
            print(f"FIGURE {entry} entry at beta2 = {c.betas[1]}, t = 2: p' worst ratio {float(ratios['p'].max()):.4f}")
        tally.add(ratios, c.n, case_name(c))
        if c.amsgrad:
            arms[0] += int((out["v"] > x["vmax"]).sum())
            arms[1] += int((out["v"] < x["vmax"]).sum())
    print(f"FIGURE {entry} coef {coef}: v' above the old vmax at {arms[0]} elements, below it at {arms[1]}")
    w = tally.report(f"{entry} coef {coef}")
    assert arms[0] > 100 and arms[1] > 100, "both arms of the amsgrad max must occur"
    assert tally.paths >= {"8-chunk", "odd 4-chunk", "scalar tail"}
    assert set(tally.worst) == {"m", "v", "vmax", "p"}
    assert w <= 1.0, tally.worst


def test_shadow_is_rne_on_ties(ops):
    """lr = 0 through the host entry leaves p as it is, so p can hold chosen bit patterns: exact ties on even and odd bf16
    neighbours, one f32 ulp off the tie, +-0, the largest value that rounds to the bf16 maximum, values across 1.0.  Every pattern
    at every position of an 8-chunk (one launch), of the odd 4-chunk and of the scalar tail (rolled launches of 7 elements)."""
    pat = R.shadow_patterns()
    L = pat.numel()
    assert math.gcd(9, L) == 1                                           # chunk k, position j holds pattern (9 k + j) mod L
    n_big = 8 * L + 4 + 3
    idx = torch.arange(n_big)
    layouts = [pat[(idx + idx // 8) % L]] + [torch.roll(pat, r)[:7] for r in range(L)]
    seen = set()
    for p in layouts:
        n = p.numel()
        c = R.Case(n=n, gdtype=F32, amsgrad=False, wd=0.0, grad_scale=1.0, betas=(0.9, 0.999), t=3, seed=0)
        x = dict(p=p.clone(), m=torch.full((n,), 1e-3), v=torch.full((n,), 1e-6), vmax=None, g=torch.full((n,), 1e-3))   # u = +0
        out, intact = run_entry(ops, "host", None, c, x, lr=0.0)
        assert intact
        assert torch.equal(out["p"].view(torch.int32), p.view(torch.int32)), "lr = 0 changed p"
        got, want = R.bf16_bits(out["shadow"]), R.bf16_rne_bits(p)
        bad = (got != want).nonzero().flatten().tolist()
        assert not bad, f"shadow of {p[bad[0]].item()!r} ({p.view(torch.int32)[bad[0]].item() & 0xFFFFFFFF:#010x}) is {got[bad[0]].item():#06x}, RNE gives " \
                        f"{want[bad[0]].item():#06x}: {R.describe(bad[0], n)}"
        codes = R.path_codes(n)
        seen |= {(int(b), int(k)) for b, k in zip(p.view(torch.int32).tolist(), codes.tolist())}
    distinct = len(set(pat.view(torch.int32).tolist()))
    assert len(seen) == 3 * distinct, "every pattern reaches the 8-chunk, the odd 4-chunk and the scalar tail"
    print(f"FIGURE shadow RNE: {distinct} patterns x 3 paths, {len(layouts)} launches, all bit-exact")


# ---------------------------------------------------------------------------------------------------------------
# fp8 mirror
# ---------------------------------------------------------------------------------------------------------------
SPAN = 2048


def launch_fp8(ops, entry, coef, p, g, m, v, vmax, shadow, state, c, w8, segs, scale, first):
    """kvq_adam_step_dev_fp8 / _guarded_fp8 on views; segs in GLOBAL elements; w8 is the mirror's element 0.  Returns the tables
    (kept alive by the caller until the synchronise)."""
    from kvq._ffi import check, io_dtype_of, lib, stream_ptr
    from kvq.engine import fp8_span_table
    total = w8.numel()
    off = torch.tensor([o for o, _ in segs], dtype=torch.int64, device="cuda")
    cnt = torch.tensor([k for _, k in segs], dtype=torch.int64, device="cuda")
    sc = torch.tensor(scale, dtype=torch.float32, device="cuda")
    span = torch.from_numpy(fp8_span_table([o for o, _ in segs], [k for _, k in segs], total, SPAN)).cuda()
    args = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), vmax.data_ptr() if vmax is not None else None, shadow.data_ptr(),
            p.numel(), io_dtype_of(g), state.data_ptr(), c.betas[0], c.betas[1], R.ADAM_EPS, c.wd, c.grad_scale, w8.data_ptr(),
            span.data_ptr(), sc.data_ptr(), off.data_ptr(), cnt.data_ptr(), len(segs), first)
    if entry == "dev_fp8":
        check(lib().kvq_adam_step_dev_fp8(*args, stream_ptr()), "kvq_adam_step_dev_fp8")
        keep = (off, cnt, sc, span)
    else:
        guard = guard_with(ops, coef)
        check(lib().kvq_adam_step_guarded_fp8(*args, guard.data_ptr(), stream_ptr()), "kvq_adam_step_guarded_fp8")
        keep = (off, cnt, sc, span, guard)
    return keep, span


def mirror_mismatches(w8, shadow, segs, scale, first):
    """Per segment: bytes of w8 (global) that are not clamp(bf16 shadow * scale, +-448) -> e4m3fn, as the mirror tests of
    tests/test_fp8_gpu.py compute them; and the number of bytes outside all segments that are no longer the sentinel."""
    bad, sat = [], 0
    inside = torch.zeros(w8.numel(), dtype=torch.bool, device=w8.device)
    for si, (o, k) in enumerate(segs):
        want = (shadow[o - first:o - first + k].float() * scale[si]).clamp(-448, 448).cpu().to(torch.float8_e4m3fn).float()
        got = w8[o:o + k].cpu().view(torch.float8_e4m3fn).float()
        bad.append(int((got != want).sum()))
        sat += int((want.abs() == 448).sum())
        inside[o:o + k] = True
    return bad, int((w8[~inside] != SENTINEL[torch.uint8]).sum()), sat


@pytest.mark.parametrize("gdtype", [F32, BF16], ids=["g-f32", "g-bf16"])
@pytest.mark.parametrize("entry,coef", [("dev_fp8", None), ("guarded_fp8", 0.37)], ids=["dev_fp8", "guarded_fp8"])
def test_fp8_mirror_combinations(ops, entry, coef, gdtype):
    """amsgrad on, f32 and bf16 gradients, a launch that starts at global element 1032 (not a multiple of 2048) inside a span no
    segment touches (-1), crosses spans that hold a segment boundary (-2) and spans wholly inside one segment, and saturation at
    +-448; then the same launch at lr = 0 on values placed around the saturation point."""
    total, first = 6 * SPAN, 1032
    n = total - first - 40
    segs = [(SPAN + 16, 1024), (2 * SPAN, 2 * SPAN), (5 * SPAN + 512, 512)]
    scale = [300.0, 2000.0, 900.0]
    c = R.Case(n=n, gdtype=gdtype, amsgrad=True, wd=0.01, grad_scale=1.0 / 3.0, betas=(0.9, 0.999), t=5, seed=41)
    assert n % 8 == 0 and first % 8 == 0 and first % SPAN != 0
    for lr in (R.LR, 0.0):
        x = R.case_inputs(c)
        if lr == 0.0:
            edge = torch.tensor([0.25, 1.0, 100.0, 0.125])          # exact in bf16; times 2000: 500, 2000, 2e5 saturate, 250 does not
            edge = torch.cat([edge, -edge])
            lo = segs[1][0] - first
            x["p"][lo:lo + 4 * edge.numel()] = edge.repeat(4)        # (no -0 among the values: -0 - (-0) would come back as +0)
        frames = {k: framed(x[k]) for k in ("p", "m", "v", "vmax")}
        frames["shadow"] = framed(n=n, dtype=BF16)
        w8_whole, w8 = framed(n=total, dtype=torch.uint8)
        g = x["g"].cuda()
        st = state_at(ops, c.t, lr, *c.betas)
        keep, span = launch_fp8(ops, entry, coef, frames["p"][1], g, frames["m"][1], frames["v"][1], frames["vmax"][1],
                                frames["shadow"][1], st, c, w8, segs, scale, first)
        torch.cuda.synchronize()
        assert span.tolist() == [-1, -2, 1, 1, -1, -2]
        assert all(frame_intact(w) for w, _ in frames.values()) and frame_intact(w8_whole), "a sentinel around a buffer changed"
        out = {k: frames[k][1].cpu() for k in frames}
        assert torch.equal(R.bf16_bits(out["shadow"]), R.bf16_rne_bits(out["p"]))
        bad, outside, sat = mirror_mismatches(w8, frames["shadow"][1], segs, scale, first)
        print(f"FIGURE {entry} g {str(gdtype)[6:]} lr {lr}: mirror mismatches per segment {bad}, bytes changed outside the segments {outside}, "
              f"{sat} expected bytes saturate at +-448")
        assert bad == [0, 0, 0] and outside == 0 and sat > 10
        if lr == 0.0:
            assert torch.equal(out["p"].view(torch.int32), x["p"].view(torch.int32)), "lr = 0 changed p"
            got = w8[segs[1][0]:segs[1][0] + 8].cpu().tolist()       # 0x7E = 448, 0x78 = 256 (250 rounded to e4m3)
            assert got == [0x7E, 0x7E, 0x7E, 0x78, 0xFE, 0xFE, 0xFE, 0xF8], [hex(b) for b in got]
        ratios = R.launch_ratios(out, x, R.case_hyper(c, coef)._replace(lr=R.f32(lr)))
        tally = Tally()
        tally.add(ratios, n, f"{entry}, lr {lr}")
        assert tally.report(f"{entry} g {str(gdtype)[6:]} lr {lr}") <= 1.0, tally.worst


# ---------------------------------------------------------------------------------------------------------------
# the production launch shape: more elements than adam_launch's block cap covers in one trip of the grid-stride loop
# ---------------------------------------------------------------------------------------------------------------
GEN_SLICE = 1 << 22
JUDGE_SLICE = 1 << 21            # about 30 f64 temporaries per judged slice: 0.5 GB


def big_inputs(n, seed, gdtype, amsgrad):
    """adam_inputs of n elements generated on the device in slices, each buffer inside a sentinel frame.  dict name -> (whole, view)."""
    frames = {k: framed(n=n, dtype=(gdtype if k == "g" else F32)) for k in ("p", "m", "v", "g") + (("vmax",) if amsgrad else ())}
    for i, s in enumerate(range(0, n, GEN_SLICE)):
        k = min(GEN_SLICE, n - s)
        x = R.adam_inputs(k, seed + i, gdtype, amsgrad, device="cuda")
        for name, (_, view) in frames.items():
            view[s:s + k] = x[name]
    return frames


def judge_big(frames, pre, hp, n, what):
    """Every element of the launch against the reference computed on the device in f64, slice by slice.  Returns (Tally, worst ratio
    over the elements of a second loop trip, arms of the max)."""
    codes = R.path_codes(n, device="cuda")
    tally, arms = Tally(), [0, 0]
    for s in range(0, n, JUDGE_SLICE):
        e = min(s + JUDGE_SLICE, n)
        x = {k: (pre[k][s:e] if k in pre else None) for k in ("p", "m", "v", "vmax")}
        x["g"] = frames["g"][1][s:e]
        out = {k: (frames[k][1][s:e] if k in frames else None) for k in ("p", "m", "v", "vmax")}
        assert torch.equal(R.bf16_bits(frames["shadow"][1][s:e]), R.bf16_rne_bits(out["p"])), f"{what}: shadow is not bf16(p') in [{s}, {e})"
        ratios = R.launch_ratios(out, x, hp)
        tally.add(ratios, n, what, first=s, codes=codes[s:e])
        if x["vmax"] is not None:
            arms[0] += int((out["v"] > x["vmax"]).sum())
            arms[1] += int((out["v"] < x["vmax"]).sum())
    return tally, tally.by_path.get("loop trip >= 2", 0.0), arms


def test_grid_stride_dev_amsgrad(ops):
    """(a) kvq_adam_step_dev, bf16 gradient, amsgrad, shadow, at n = one full trip of the capped grid (32768 blocks x 256 threads x 8
    elements, adam_launch's cap) + 1000 chunks of a second trip + the odd 4-chunk + a 3-element tail."""
    n = R.ADAM_TRIP + 8 * 1000 + 4 + 3
    c = R.Case(n=n, gdtype=BF16, amsgrad=True, wd=0.01, grad_scale=1.0 / 3.0, betas=(0.9, 0.999), t=5, seed=1000)
    codes = R.path_codes(n)
    assert [int((codes == k).sum()) for k in range(4)] == [R.ADAM_TRIP, 4, 3, 8000], "elements on a second loop trip must exist"
    del codes
    frames = big_inputs(n, c.seed, c.gdtype, True)
    frames["shadow"] = framed(n=n, dtype=BF16)
    pre = {k: frames[k][1].clone() for k in ("p", "m", "v", "vmax")}
    g0 = frames["g"][1].clone()
    st = state_at(ops, c.t, R.LR, *c.betas)
    ops.adam_step_dev(frames["p"][1], frames["g"][1], frames["m"][1], frames["v"][1], st, beta1=c.betas[0], beta2=c.betas[1], eps=R.ADAM_EPS,
                      weight_decay=c.wd, vmax=frames["vmax"][1], shadow=frames["shadow"][1], grad_scale=c.grad_scale)
    torch.cuda.synchronize()
    assert all(frame_intact(w) for w, _ in frames.values()), "a sentinel around a buffer changed"
    assert torch.equal(g0.view(torch.int16), frames["g"][1].view(torch.int16))
    tally, second, arms = judge_big(frames, pre, R.case_hyper(c), n, "grid-stride dev")
    print(f"FIGURE grid-stride dev: worst ratio on the second loop trip {second:.4f}; v' above the old vmax at {arms[0]} elements, below at {arms[1]}")
    w = tally.report("grid-stride dev")
    assert tally.paths == set(R.PATHS) and arms[0] > 1000 and arms[1] > 1000
    assert 0.0 < second <= 1.0 and w <= 1.0, tally.worst


def test_grid_stride_dev_fp8(ops):
    """(b) kvq_adam_step_dev_fp8 at n = 8 (32768 x 256 + 1000): segments in the first span, across local element 67,108,864 (where
    the threads' second trip starts) and at the end; mirror bytes and the master judged."""
    n = 8 * (R.ADAM_BLOCK_CAP * 256 + 1000)
    first = 16
    total = first + n
    segs = [(first + 16, 1024), (first + R.ADAM_TRIP - 4096, 8192 + 48), (total - 1024, 1024)]
    scale = [300.0, 2000.0, 900.0]
    assert all(o % 16 == 0 and k % 16 == 0 for o, k in segs) and segs[1][0] - first < R.ADAM_TRIP < segs[1][0] + segs[1][1] - first
    c = R.Case(n=n, gdtype=F32, amsgrad=False, wd=0.0, grad_scale=1.0, betas=(0.9, 0.999), t=2, seed=2000)
    frames = big_inputs(n, c.seed, c.gdtype, False)
    frames["shadow"] = framed(n=n, dtype=BF16)
    w8_whole, w8 = framed(n=total, dtype=torch.uint8)
    pre = {k: frames[k][1].clone() for k in ("p", "m", "v")}
    st = state_at(ops, c.t, R.LR, *c.betas)
    keep, span = launch_fp8(ops, "dev_fp8", None, frames["p"][1], frames["g"][1], frames["m"][1], frames["v"][1], None, frames["shadow"][1],
                            st, c, w8, segs, scale, first)
    torch.cuda.synchronize()
    assert all(frame_intact(w) for w, _ in frames.values()) and frame_intact(w8_whole), "a sentinel around a buffer changed"
    bad, outside, sat = mirror_mismatches(w8, frames["shadow"][1], segs, scale, first)
    print(f"FIGURE grid-stride dev_fp8: mirror mismatches per segment {bad}, bytes changed outside the segments {outside}, {sat} saturated")
    assert bad == [0, 0, 0] and outside == 0 and sat > 10
    tally, second, _ = judge_big(frames, pre, R.case_hyper(c), n, "grid-stride dev_fp8")
    print(f"FIGURE grid-stride dev_fp8: worst ratio on the second loop trip {second:.4f}")
    w = tally.report("grid-stride dev_fp8")
    assert tally.paths == {"8-chunk", "loop trip >= 2"}
    assert 0.0 < second <= 1.0 and w <= 1.0, tally.worst


# ---------------------------------------------------------------------------------------------------------------
# step state
# ---------------------------------------------------------------------------------------------------------------
PAD_WORD = 0x1234ABCD


def milestone_sets(t):
    """0, 1, 3 and 8 milestones; t - 1 equal to a milestone, one below it and one above it."""
    lo = max(t - 4, 0)
    return [[], [t - 1], [t], [max(t - 2, 0)], [max(t - 2, 0), t - 1, t + 5], list(range(lo, lo + 8))]


def test_step_state_parity(ops):
    from kvq._ffi import lib, stream_ptr
    worst, where, launches = [0.0, 0.0, 0.0], [None] * 3, 0
    for t in (1, 2, 10, 1000, 10 ** 6, 2 ** 32 + 5):
        for ms in milestone_sets(t):
            for gamma in (0.1, 0.5):
                for b1, b2 in R.AXES["betas"]:
                    whole, st = framed(n=3, dtype=torch.int64)
                    st.copy_(torch.tensor([t - 1, 0, PAD_WORD << 32], dtype=torch.int64))
                    ops.step_state_advance(st, 1e-3, gamma, ms, b1, b2)
                    raw = st.cpu()
                    launches += 1
                    what = f"t = {t}, milestones {ms}, gamma {gamma}, betas ({b1}, {b2})"
                    assert frame_intact(whole) and int(raw[0]) == t, f"{what}: step count {int(raw[0])}"
                    assert (int(raw[2]) >> 32) & 0xFFFFFFFF == PAD_WORD, f"{what}: the pad word changed"
                    got = raw[1:].view(torch.float32)[:3].tolist()
                    for i, r in enumerate(R.step_state_ratios(got, R.step_state_ref(t, 1e-3, gamma, ms, b1, b2))):
                        if r > worst[i]:
                            worst[i], where[i] = r, what
    for name, w, at in zip(("lr", "bc1", "bc2s"), worst, where):
        print(f"FIGURE step state {name}: worst ratio {w:.4f} at {at} ({launches} launches)")
    assert max(worst) <= 1.0, (worst, where)
    # nine milestones are refused and leave the state alone
    st = ops.new_step_state("cuda")
    st[0] = 4
    arr = (ctypes.c_int64 * 9)(*range(9))
    assert lib().kvq_step_state_advance(st.data_ptr(), 1e-3, 0.1, arr, 9, 0.9, 0.999, stream_ptr()) == -1
    assert b"at most 8 milestones" in lib().kvq_last_error()
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [4, 0, 0]
