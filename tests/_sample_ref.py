"""f64 reference of top-k / top-p filtered sampling (kvq_gen_select_filtered, include/kvq.h) on host tensors --
the checker of tests/test_sample_ref.py, tests/test_sample_kernels_gpu.py and tests/test_sample_engine_gpu.py.  Plain torch.

Everything starts from y = fl32(logit * inv_tau), formed on the CPU by y_of(): one IEEE multiply, so exactly the kernel's product.

  ORDER   v before w iff y_v > y_w, or y_v == y_w and v < w; a NaN is never kept and never counted (it sorts behind everything).
  top-k   K = the first min(top_k, n_valid) of the order (top_k <= 0: every valid column).
  top-p   inside K: m = max y, e = exp(y - m), Z = sum over K, C_j = mass of the first j; n_keep = the smallest j >= 1 with
          C_j >= top_p Z (TopPLogitsWarper's rule: the token that crosses p is kept); top_p outside (0, 1): off.
  score   log p~(c) = y_c - m - log C_n_keep, p~ = the distribution sampled from.

The two tolerances are DERIVED from the kernel's own summation order (the count is written out in include/kvq.h), not tuned:
  TOL_MASS  = 2^-17, relative to Z.  A mass is summed through 16 roundings (a thread's 8 columns as a tree: 3, its 4 chunks: 3,
              the wave's butterfly: 6, the tree over 16 waves: 4); C_j adds at most 32 such sums, one per bit of the search (32),
              and j e_T (2): 50 roundings of at most 2^-24 of a partial sum <= Z each.  Every term carries the rounding of y - m
              (2^-24 |y - m| relative; weighted by e / Z and summed this is at most 2^-24 (H - log Z) <= 2^-24 log V <= 10.4 2^-24
              for V <= 32768, H the entropy) and expf's ulp (2 2^-24).  So |C_j - exact| <= 62.4 2^-24 Z, the same for Z, one more
              rounding for fl(top_p Z): the kernel's comparison is an exact comparison at some p' with
              |p' - top_p| <= (2 * 62.4 + 1) 2^-24 < 128 2^-24 = 2^-17.  Hence keep_band(): n_keep must lie between the exact
              n_keep at top_p - TOL_MASS and at top_p + TOL_MASS.
  LOGPROB   |got - exact| <= 2^-17 + 2^-22 (|y_c - m| + |log C|): C >= 1 (the maximum is kept) carries the same 62.4 2^-24 < 2^-18
              relative error, logf adds an ulp of |log C|, the two subtractions half an ulp of their results each.
"""
from __future__ import annotations

import math
import struct

import torch

TOL_MASS = 2.0 ** -17
LOGPROB_ABS = 2.0 ** -17
LOGPROB_REL = 2.0 ** -22


def f32(x):
    """the f32 nearest to the Python float x, as a Python float: what a state word holds"""
    return struct.unpack("<f", struct.pack("<f", float(x)))[0]


def y_of(logits, temperature):
    """[B, V] logits (any float dtype, on the CPU) -> y = fl32(logit * fl32(1 / temperature)); temperature 0 (greedy): the logits"""
    x = logits.detach().float().cpu()
    if not temperature > 0:
        return x.clone()
    return x * torch.tensor(f32(1.0 / float(temperature)), dtype=torch.float32)


def order_of(y):
    """-> (order [B, V] int64: the columns of every row in the order, NaNs last; n_valid [B])"""
    nan = y.isnan()
    yd = torch.where(nan, torch.full_like(y, float("-inf")), y).double()
    o1 = torch.sort(yd, dim=1, descending=True, stable=True).indices
    o2 = torch.sort(nan.gather(1, o1).long(), dim=1, stable=True).indices
    return o1.gather(1, o2), (~nan).sum(dim=1)


def rank_of(order):
    """rank [B, V]: rank[b, v] = the place of column v in the order of row b"""
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(order.shape[1]).unsqueeze(0).expand_as(order).contiguous())
    return rank


class Cut:
    """The reference of a batch of rows y [B, V] f32 under (top_k, top_p): order, rank, n_valid, kk = |K|, m, C [B, V] (cumulative
    f64 mass in the order, inside K), Z, n_keep [B], cut [B] (-1 when nothing is kept), logC [B]."""

    def __init__(self, y, top_k=0, top_p=1.0, greedy=False):
        self.y = y
        B, V = y.shape
        self.order, self.n_valid = order_of(y)
        self.rank = rank_of(self.order)
        if greedy:
            top_k, top_p = 0, 1.0
        self.kk = self.n_valid if top_k <= 0 else torch.clamp(self.n_valid, max=int(top_k))
        ys = y.gather(1, self.order).double()
        place = torch.arange(V).unsqueeze(0)
        inside = place < self.kk.unsqueeze(1)
        self.m = ys[:, 0].clone()
        e = torch.where(inside, torch.exp(ys - self.m.unsqueeze(1)), torch.zeros_like(ys))
        self.C = torch.cumsum(e, dim=1)
        self.Z = self.C[:, -1].clone()
        p = f32(top_p) if isinstance(top_p, (int, float)) else float("nan")
        self.p = p if 0.0 < p < 1.0 else None
        self.n_keep = self.n_keep_at(self.p)
        last = (self.n_keep - 1).clamp(min=0).unsqueeze(1)
        self.cut = torch.where(self.n_keep > 0, self.order.gather(1, last).squeeze(1), torch.full_like(self.n_keep, -1))
        self.logC = torch.log(self.C.gather(1, last).squeeze(1))

    def n_keep_at(self, p):
        """the smallest j >= 1 with C_j >= p Z inside K (|K| if none); p None: |K|; p <= 0: 1"""
        if p is None:
            return self.kk.clone()
        if p <= 0.0:
            return torch.clamp(self.kk, max=1)
        j = torch.searchsorted(self.C, (p * self.Z).unsqueeze(1), right=False).squeeze(1) + 1
        return torch.minimum(j, self.kk)

    def keep_band(self, tol=TOL_MASS):
        """(n_keep at top_p - tol, n_keep at top_p + tol): what a comparison decided within tol of top_p may answer"""
        if self.p is None:
            return self.kk.clone(), self.kk.clone()
        return self.n_keep_at(self.p - tol), self.n_keep_at(self.p + tol)

    def kept(self, n_keep=None):
        """[B, V] bool: the first n_keep (default: the reference's) of the order"""
        n = self.n_keep if n_keep is None else n_keep
        return (self.rank < n.unsqueeze(1)) & ~self.y.isnan()

    def logprob(self, choice, n_keep=None):
        """(log p~(choice) [B] f64 under the first n_keep of the order, bound [B]: LOGPROB_ABS + LOGPROB_REL (|y_c - m| + |log C|))"""
        n = self.n_keep if n_keep is None else n_keep
        logC = torch.log(self.C.gather(1, (n - 1).clamp(min=0).unsqueeze(1)).squeeze(1))
        d = self.y.gather(1, choice.long().unsqueeze(1)).squeeze(1).double() - self.m
        return d - logC, LOGPROB_ABS + LOGPROB_REL * (d.abs() + logC.abs())

    def probs(self):
        """[B, V] f64: the renormalised distribution over the reference's kept set"""
        e = torch.exp(self.y.double() - self.m.unsqueeze(1))
        e = torch.where(self.kept(), e, torch.zeros_like(e))
        return e / e.sum(dim=1, keepdim=True)


def keep_band(y, top_k, top_p, tol=TOL_MASS):
    return Cut(y, top_k, top_p).keep_band(tol)


def masked_logits(logits, kept):
    """the logits with every column outside the kept set at -inf: what kvq_gen_select must choose the same token from"""
    return torch.where(kept.to(logits.device), logits, torch.full_like(logits, float("-inf")))


def chain_roundings():
    """the count behind TOL_MASS, spelled out: (per mass sum, per C_j, total in units of 2^-24 for the comparison)"""
    per_sum = 3 + 3 + 6 + 4
    per_c = per_sum + 32 + 2
    per_side = per_c + 10.4 + 2.0
    return per_sum, per_c, 2 * per_side + 1


assert chain_roundings()[2] * 2.0 ** -24 <= TOL_MASS and math.log(32768) <= 10.4
