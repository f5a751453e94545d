"""Plain Python restatement of the free-running reconstruction metrics (include/kvq.h "free-running reconstruction metrics",
csrc/kvq_seqcmp.hip): the two-row Levenshtein DP the kernel is read against line by line, the per-sentence record, the table sums
and an exhaustive brute-force distance for tiny inputs.  Test infrastructure only; integers throughout, nothing is toleranced."""
from __future__ import annotations

from functools import lru_cache

import numpy as np


def edit_distance(h, r) -> int:
    """Levenshtein distance of the sequences h and r, unit costs, two rows of the table."""
    h, r = [int(x) for x in h], [int(x) for x in r]
    prev = list(range(len(r) + 1))                   # D[0][j] = j
    for i in range(1, len(h) + 1):
        cur = [i] + [0] * len(r)                     # D[i][0] = i
        for j in range(1, len(r) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (h[i - 1] != r[j - 1]))
        prev = cur
    return prev[len(r)]


def brute_force_distance(h, r) -> int:
    """The same by definition: the cheapest way to use up both sequences with deletions, insertions, substitutions and free
    matches, searched exhaustively (for sequences of a few tokens)."""
    h, r = tuple(int(x) for x in h), tuple(int(x) for x in r)

    @lru_cache(maxsize=None)
    def go(i, j):
        if i == len(h):
            return len(r) - j
        if j == len(r):
            return len(h) - i
        return min(go(i + 1, j) + 1, go(i, j + 1) + 1, go(i + 1, j + 1) + (h[i] != r[j]))
    return go(0, 0)


def positional_hits(h, r) -> int:
    return sum(1 for a, b in zip(h, r) if int(a) == int(b))


def seq_compare(hyp, hyp_len, ref, ref_len, hyp_skip=0, Lmax=128):
    """(out [B, 4] int32, n_bad) as kvq_seq_compare leaves them.  hyp, ref: [B, L] integer arrays (any row may be longer than its
    length says: what lies behind is not a token)."""
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    B = hyp.shape[0]
    out = np.zeros((B, 4), dtype=np.int32)
    bad = 0
    for b in range(B):
        n, m = int(hyp_len[b]) - int(hyp_skip), int(ref_len[b])
        if not (0 <= n <= Lmax and 0 <= m <= Lmax) or hyp_skip + n > hyp.shape[1] or m > ref.shape[1]:
            out[b] = (-1, 0, 0, 0)
            bad += 1
            continue
        h, r = hyp[b, hyp_skip:hyp_skip + n].tolist(), ref[b, :m].tolist()
        out[b] = (edit_distance(h, r), positional_hits(h, r), n, m)
    return out, bad


def accumulate(per, slot, table):
    """table [R, 6] int64 += (1, dist == 0, dist, hits, n, m) at every slot inside [0, R) of every sentence with dist >= 0: a numpy
    scatter-add (np.add.at).  Returns the table."""
    per, slot = np.asarray(per, dtype=np.int64), np.asarray(slot, dtype=np.int64)
    R = table.shape[0]
    rec = np.stack([np.ones(len(per), dtype=np.int64), (per[:, 0] == 0).astype(np.int64), per[:, 0], per[:, 1], per[:, 2], per[:, 3]], axis=1)
    for c in range(slot.shape[1]):
        ok = (per[:, 0] >= 0) & (slot[:, c] >= 0) & (slot[:, c] < R)
        np.add.at(table, slot[ok, c], rec[ok])
    return table
