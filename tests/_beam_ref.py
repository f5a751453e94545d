"""f64 reference and judges of beam search: of kvq_beam_select / kvq_beam_gather (csrc/kvq_generate.hip) and of
TrainEngine.beam_search -- the checkers of tests/test_beam_ref.py (CPU), tests/test_beam_kernels_gpu.py and
tests/test_beam_engine_gpu.py.  numpy and torch on the host, no device needed.

Slot space (include/kvq.h "beam search"): beam w of sentence b is row r = b W + w.  A state is a dict of numpy arrays
    ids [R, L] int64, parent [R, L] int32, step_scores [R, L] f32, anc [2, R, L] int32, scores [R] f32, finished [R], lengths [R] int32

candidates      the scored candidates of one sentence at one step, in f64 ON THE KERNEL'S OWN f32 INPUTS (the logits as the kernel
                read them, the incoming f32 scores), best first: larger s, then lower beam, then lower token
score_tol       the tolerance of a candidate's score against that reference (derivation below)
is_decided      whether a (sentence, step) may be compared token for token
book            the bookkeeping of a step as a function of the choices (parent beam, token, score) -- exact, no arithmetic
step_ref        candidates + book: the reference's own step
gather_ref      kvq_beam_gather;  backtrack: a hypothesis from ids and parent alone

Tolerance of a step's score, |s - ref| <= 2^-15 + 2^-22 (|lse| + |lp| + |s|):
  s = fl(score + fl(x - lse)), lse = fl(m + log(sum_v exp(x_v - m))) in f32.  The second term is one rounding each of lse, lp and s
  (2^-24 relative each), doubled.  The first bounds the error of lse before its own rounding, as an absolute error of
  log(sum): a term reaches the sum through at most 256 f32 roundings (the kernel refuses a vocabulary that would need more.  Its
  online form: the term's exponential, 2 ulp; a tree of depth 3 over the 8 columns of a chunk; per further chunk of the thread one
  addition and at most one rescaling of the running sum by a fast exponential, 3; then the 6 levels of a wave and the 2 .. 16
  waves of a beam, an exponential, a product and an addition each, 4: 4 chunks + 5 + 4 (6 + waves), which is 4 * 30 + 5 + 32 = 157
  for V = 30522 with W = 8 and 4 * 4 + 5 + 88 = 109 with W = 1), each 2^-24 relative to a partial sum that is no larger than the
  total: 256 * 2^-24 = 2^-16 relative to the sum, i.e. 2^-16 absolute in its logarithm; the fast exponential's argument scaling,
  |x - m| log2(e) rounded to f32, moves a term by at most 100 * 1.44 * 2^-24 < 2^-16.8 relative at |x - m| up to 100 (the figure of
  tests/_gen_ref.py; the arguments of a term's rescalings add up to no more than its distance from the final maximum, so the
  online form stays inside the same figure); logf adds 2 ulp of log(sum) <= 2^-22 * 12.
  2^-16 + 2^-16.8 + 2^-18.4 < 2^-15.  Derived, not tuned.

Decided: the reference's best W + 1 candidates are pairwise more than twice the tolerance apart (neighbours of the sorted list:
twice the larger of the two tolerances), so that no admissible error of the scores changes which W are chosen, or their order.
"""
from __future__ import annotations

import numpy as np
import torch

TOL_ABS = 2.0 ** -15
TOL_REL = 2.0 ** -22
NEG_INF = float("-inf")


def round_up(x, a):
    return (x + a - 1) // a * a


def score_tol(lse, lp, s):
    return TOL_ABS + TOL_REL * (abs(lse) + abs(lp) + abs(s))


def new_state(B, W, L, prompt, pad, R=None):
    """The start of a search as TrainEngine._gen_reset / _beam_reset (kvq/inference.py) set it: prompt [B, P] int64 (numpy or torch)."""
    prompt = np.asarray(prompt, dtype=np.int64)
    R = round_up(B * W, 8) if R is None else R
    own = np.arange(R, dtype=np.int32)
    ids = np.full((R, L), pad, dtype=np.int64)
    ids[:B * W, :prompt.shape[1]] = np.repeat(prompt, W, axis=0)
    scores = np.full(R, NEG_INF, dtype=np.float32)
    scores[:B * W:W] = 0.0
    finished = np.zeros(R, dtype=np.int32)
    finished[B * W:] = 1
    return dict(ids=ids, parent=np.repeat(own[:, None], L, axis=1), step_scores=np.zeros((R, L), dtype=np.float32),
                anc=np.repeat(np.repeat(own[:, None], L, axis=1)[None], 2, axis=0).copy(), scores=scores, finished=finished,
                lengths=np.full(R, L, dtype=np.int32))


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def lse64(x):
    """log sum exp of a 1-D f64 array; NaN if any element is, -inf for an empty sum"""
    x = np.asarray(x, dtype=np.float64)
    if np.isnan(x).any():
        return float("nan")
    m = x.max()
    if not np.isfinite(m):
        return float(m) if m < 0 else float("nan")          # all -inf: -inf; a +inf: inf - inf
    return float(m + np.log(np.exp(x - m).sum()))


def candidates(state, x, V, W, b, keep=None):
    """The candidates of sentence b, best first: dicts(s (f64), w, v, tol, lse, fin).  x [R, >= V]: the logits the kernel read, any
    float array (upcast exactly).  keep: how many to return (default W + 1); a live beam contributes its best `keep`."""
    keep = W + 1 if keep is None else keep
    R = state["scores"].shape[0]
    out = []
    for w in range(min(W, R - b * W)):
        r = b * W + w
        score = float(state["scores"][r])
        if not score > NEG_INF:
            continue                                                    # a dead beam offers nothing
        if state["finished"][r]:
            out.append(dict(s=score, w=w, v=0, tol=score_tol(0.0, 0.0, score), lse=0.0, fin=True))
            continue
        row = np.asarray(x[r, :V], dtype=np.float64)
        lse = lse64(row)
        if not np.isfinite(lse):
            continue                                                    # a NaN (or +inf) among the columns: nothing to offer
        s = score + (row - lse)
        order = np.argsort(-s, kind="stable")[:keep]                    # stable: equal scores in ascending v
        for v in order:
            if s[v] > NEG_INF:
                out.append(dict(s=float(s[v]), w=w, v=int(v), tol=score_tol(lse, row[v] - lse, s[v]), lse=lse, fin=False))
    out.sort(key=lambda c: (-c["s"], c["w"], c["v"]))
    return out[:keep]


def is_decided(cands, W):
    top = cands[:W + 1]
    return all(top[i]["s"] - top[i + 1]["s"] > 2.0 * max(top[i]["tol"], top[i + 1]["tol"]) for i in range(len(top) - 1))


def ref_score(state, x, V, W, b, w, v, fin):
    """(s, tol) of the candidate (beam w, token v) of sentence b in f64 -- what a kernel's choice is judged against"""
    r = b * W + w
    score = float(state["scores"][r])
    if fin:
        return score, score_tol(0.0, 0.0, score)
    row = np.asarray(x[r, :V], dtype=np.float64)
    lse = lse64(row)
    s = score + (row[v] - lse)
    return float(s), score_tol(lse, row[v] - lse, s)


def book(state, choices, W, t, P, eos_id, pad_id):
    """The state after position t + 1 was chosen.  choices[b] = list of (w, v, s) for new beams 0 .. of sentence b, best first (w: the
    parent beam; v: the token, ignored for a finished parent; s: the score); shorter than the sentence's rows: dead beams follow.
    Nothing changes unless 0 <= t and t + 1 < L.  Scores are stored as f32 (exact for scores that are f32 already)."""
    new = copy_state(state)
    R, L = state["ids"].shape
    if t < 0 or t + 1 >= L:
        return new
    old, nxt = state["anc"][t & 1], new["anc"][(t + 1) & 1]
    if t + 1 < P:
        for r in range(R):
            nxt[r, :t + 1] = old[r, :t + 1]
            nxt[r, t + 1] = r
            new["parent"][r, t + 1] = r
            new["step_scores"][r, t + 1] = state["scores"][r]
        return new
    for b in range(-(-R // W)):
        nW = min(W, R - b * W)
        for i in range(nW):
            r = b * W + i
            if i >= len(choices[b]):
                new["ids"][r, t + 1] = pad_id
                new["parent"][r, t + 1] = r
                new["scores"][r] = new["step_scores"][r, t + 1] = NEG_INF
                new["finished"][r] = 1
                src = r
            else:
                w, v, s = choices[b][i]
                src = b * W + w
                was = bool(state["finished"][src])
                new["ids"][r, t + 1] = pad_id if was else v
                new["parent"][r, t + 1] = src
                new["scores"][r] = new["step_scores"][r, t + 1] = s
                ends = (not was) and eos_id is not None and v == eos_id
                new["finished"][r] = 1 if (was or ends) else 0
                new["lengths"][r] = t + 2 if ends else state["lengths"][src]
            nxt[r, :t + 1] = old[src, :t + 1]
            nxt[r, t + 1] = r
    return new


def step_ref(state, x, V, W, t, P, eos_id, pad_id):
    """The reference's own step -> (new state, per sentence: the candidate list (W + 1 best), decided).  Inside the prompt the lists
    are empty and every sentence is decided."""
    R, L = state["ids"].shape
    S = -(-R // W)
    if t < 0 or t + 1 >= L or t + 1 < P:
        return book(state, None, W, t, P, eos_id, pad_id), [[] for _ in range(S)], [True] * S
    cands = [candidates(state, x, V, W, b) for b in range(S)]
    choices = [[(c["w"], c["v"], c["s"]) for c in cs[:W]] for cs in cands]
    return book(state, choices, W, t, P, eos_id, pad_id), cands, [is_decided(cs, W) for cs in cands]


def choices_of(new, W, t):
    """What a kernel chose at step t, read from its state after the step: per sentence [(w, v, s, dead)] for every row"""
    R = new["ids"].shape[0]
    out = []
    for b in range(-(-R // W)):
        rows = []
        for i in range(min(W, R - b * W)):
            r = b * W + i
            s = float(new["step_scores"][r, t + 1])
            rows.append((int(new["parent"][r, t + 1]) - b * W, int(new["ids"][r, t + 1]), s, not s > NEG_INF))
        out.append(rows)
    return out


def judge_choices(old, got, x, V, W, t, eos_id, pad_id):
    """A free step's choices against the reference.  got[b] = [(w, v, s, dead)] per row of sentence b (choices_of).  Asserts (1) on
    decided sentences the chosen (parent, token) are the reference's, (2) every chosen score is within score_tol of the f64 score of
    THAT candidate, (3) live beams come first and are as many as there are candidates.
    -> (decided flags, worst |s - ref| / tol, the choices as book() takes them)."""
    _, cands, decided = step_ref(old, x, V, W, t, 0, eos_id, pad_id)
    worst, replay = 0.0, []
    for b, rows in enumerate(got):
        live = [(w, v, s) for (w, v, s, dead) in rows if not dead]
        assert all(dead for (_, _, _, dead) in rows[len(live):]), f"sentence {b}: a dead beam in front of a live one"
        assert len(live) == min(len(rows), len(candidates(old, x, V, W, b, keep=len(rows)))), f"sentence {b}: number of live beams"
        for i, (w, v, s) in enumerate(live):
            assert 0 <= w < len(rows) and float(old["scores"][b * W + w]) > NEG_INF, f"sentence {b} beam {i}: parent {w} is no live row"
            fin = bool(old["finished"][b * W + w])
            ref, tol = ref_score(old, x, V, W, b, w, 0 if fin else v, fin)
            worst = max(worst, abs(s - ref) / tol)
            assert abs(s - ref) <= tol, f"sentence {b} beam {i}: score {s!r} against {ref!r}, tolerance {tol:.3e}"
            if decided[b]:
                c = cands[b][i]
                assert (w, fin) == (c["w"], c["fin"]) and (fin or v == c["v"]), f"sentence {b} beam {i}: chose {(w, v)}, reference {(c['w'], c['v'])}"
        replay.append([(w, v, np.float32(s)) for (w, v, s) in live])
    return decided, worst, replay


def judge_step(old, new, x, V, W, t, P, eos_id, pad_id):
    """A kernel's step against the reference: old -> new over the logits x.  judge_choices on what the kernel chose, and the whole new
    state is book(old, the kernel's own choices) -- exactly.  -> (decided flags, worst |s - ref| / tol)."""
    R, L = old["ids"].shape
    decided, worst, replay = [True] * -(-R // W), 0.0, None
    if 0 <= t and P <= t + 1 < L:
        decided, worst, replay = judge_choices(old, choices_of(new, W, t), x, V, W, t, eos_id, pad_id)
    want = book(old, replay, W, t, P, eos_id, pad_id)
    for k in old:
        assert np.array_equal(new[k], want[k], equal_nan=True), f"bookkeeping: {k}"
    return decided, worst


def gather_ref(state, t, pad_id):
    """kvq_beam_gather: out[r, j] = ids[anc[t & 1][r, j], j] for j < lengths[r] (and j <= t), pad_id behind"""
    R, L = state["ids"].shape
    out = np.full((R, L), pad_id, dtype=np.int64)
    for r in range(R):
        for j in range(min(int(state["lengths"][r]), t + 1, L)):
            out[r, j] = state["ids"][state["anc"][t & 1][r, j], j]
    return out


def backtrack(ids, parent, r, t):
    """the tokens 0 .. t of the beam living in row r after position t, through `parent` alone"""
    out = np.zeros(t + 1, dtype=np.int64)
    for j in range(t, -1, -1):
        out[j] = ids[r, j]
        r = int(parent[r, j])
    return out


def state_to(state, device):
    return {k: torch.from_numpy(v.copy()).to(device) for k, v in state.items()}


def state_from(tensors):
    return {k: v.detach().cpu().numpy().copy() for k, v in tensors.items()}


# ---- the random cases of kvq_beam_select (tests/test_beam_kernels_gpu.py), seeds chosen on the CPU (tests/test_beam_ref.py) ----------
def select_case(V, ld, B, W, dtype, seed, L=8, t=5):
    """A search in the middle: position t of L, every beam of the B sentences alive with a random f32 score and a random history
    inside its sentence, beam 1 of sentence 1 finished (it competes with its score alone); R = round_up(B W, 8), the rows behind
    B W dead.  Logits 2.5 N(0, 1) rounded to `dtype`, the columns behind V at +3e38 (they must never win).
    -> (state, logits [R, ld] `dtype` on the CPU, t)"""
    g = np.random.default_rng(seed)
    st = new_state(B, W, L, g.integers(0, V, (B, 1)), 0)
    R, n = st["ids"].shape[0], B * W
    st["scores"][:n] = (-5.0 * g.random(n)).astype(np.float32)
    st["ids"][:n, :t + 1] = g.integers(0, V, (n, t + 1))
    sentence = (np.arange(n) // W * W)[:, None]
    for half in (0, 1):
        st["anc"][half][:n, :t + 1] = sentence + g.integers(0, W, (n, t + 1))
    st["anc"][t & 1][:n, t] = np.arange(n)                              # position t of a beam's history is its own row
    st["parent"][:n, 1:t + 1] = sentence + g.integers(0, W, (n, t))
    st["step_scores"][:n, 1:t + 1] = (-5.0 * g.random((n, t))).astype(np.float32)
    if W >= 2 and B >= 2:
        st["finished"][W + 1], st["lengths"][W + 1], st["scores"][W + 1] = 1, 3, np.float32(-0.5)
    x = torch.from_numpy((2.5 * g.standard_normal((R, ld))).astype(np.float32))
    x[:, V:] = 3e38
    return st, x.to(dtype), t


SELECT_SHAPES = [(37, 40, 3), (2048, 2048, 3)]                           # (V, ld, B), each with W in SELECT_BEAMS and both dtypes
SELECT_BEAMS = [1, 2, 3, 8]
SELECT_LARGE = (30522, 30528, 2, 4)                                      # (V, ld, B, W)


def select_cases():
    """[(V, ld, B, W, dtype)] of the random-case test"""
    cases = [(V, ld, B, W, dt) for (V, ld, B) in SELECT_SHAPES for W in SELECT_BEAMS for dt in (torch.float32, torch.bfloat16)]
    return cases + [SELECT_LARGE + (dt,) for dt in (torch.float32, torch.bfloat16)]


def select_seed(V, W, dtype):
    return SELECT_SEEDS.get((V, W, str(dtype).split(".")[-1]), 0)


# seed per (V, W, dtype): the first of 0, 1, 2, ... whose B sentences are all decided by the numpy reference (tests/test_beam_ref.py
# recomputes the share: it must stay at or below 5 %; bf16 logits tie often -- 8 significant bits -- hence the search)
SELECT_SEEDS = {(2048, 8, "bfloat16"): 5}                             # every other case: seed 0


def chain_logits(R, V, steps, dtype, seed=4):
    """the logits of the chained-steps test, one [R, V] tensor per step (seed 4: every step decided in f32 and in bf16, tests/test_beam_ref.py)"""
    g = torch.Generator().manual_seed(seed)
    return [(2.5 * torch.randn((R, V), generator=g)).to(dtype) for _ in range(steps)]
