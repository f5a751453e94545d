"""numpy restatement of the codebook revival (include/kvq.h "codebook revival"; csrc/kvq_vq_revive.hip), test infrastructure only.

One step = usage flags -> idle counters -> donor draw (Philox4x32-10, transcribed from csrc/kvq_common.h) -> rows -> apply.  Every
quantity is an integer or a copied float: the kernels are compared against this bit for bit."""
import numpy as np

SITE = 0x52455649
INT32_MAX = 2**31 - 1
_M32 = 0xFFFFFFFF


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10, one block: philox4x32() of csrc/kvq_common.h on python integers."""
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _M32, p1 & _M32, ((p0 >> 32) ^ c3 ^ k1) & _M32, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def draw(seed, c, N, world=1):
    """(owner rank, donor token) of code c = g K + k: drop_bits(seed, SITE, c) of csrc/kvq_common.h."""
    seed, c, N, world = int(seed) & 0xFFFFFFFFFFFFFFFF, int(c), int(N), int(world)        # python integers: no wrap-around
    x, y, _z, _w = philox4x32(c & _M32, (c >> 32) & _M32, SITE, 0x5EED, seed & _M32, seed >> 32)
    return y % world, (x * N) >> 32


def usage_flags(idx, K):
    """idx [G, N] int64 -> used [G, K] int32; indices outside [0, K) are ignored."""
    idx = np.asarray(idx).reshape(idx.shape[0], -1)
    used = np.zeros((idx.shape[0], K), np.int32)
    for g in range(idx.shape[0]):
        ok = idx[g][(idx[g] >= 0) & (idx[g] < K)]
        used[g, ok] = 1
    return used


def advance(idle, used):
    """idle' = used ? 0 : min(idle + 1, INT32_MAX)"""
    nxt = np.minimum(idle.astype(np.int64) + 1, INT32_MAX).astype(np.int32)
    return np.where(used != 0, np.int32(0), nxt).astype(np.int32)


def select(z_by_rank, used, idle, T, seed, rank=None):
    """z_by_rank: list (one entry per rank) of [G, N, D] float32 arrays holding the exact f32 values of the io-dtype z.
    Returns (idle', dead [G, K] bool, rows [G, K, D] f32, owner [G, K], token [G, K]).  rank = None: the rows after the SUM
    all-reduce (the owner's row; + 0.0 when world > 1); rank = r: what rank r's select kernel writes (zeros unless it owns the code).
    Rows of codes that are not dead are NaN here: the kernels do not write them."""
    world = len(z_by_rank)
    G, N, D = z_by_rank[0].shape
    K = used.shape[1]
    idle2 = advance(idle, used)
    dead = idle2 >= T
    rows = np.full((G, K, D), np.nan, np.float32)
    owner = np.full((G, K), -1, np.int64)
    token = np.full((G, K), -1, np.int64)
    for g, k in zip(*np.nonzero(dead)):
        o, n = draw(seed, g * K + k, N, world)
        owner[g, k], token[g, k] = o, n
        if rank is None:
            rows[g, k] = z_by_rank[o][g, n]
            if world > 1:
                rows[g, k] = rows[g, k] + np.float32(0.0)          # -0.0 + 0.0 = +0.0: what the sum with the other ranks' zeros gives
        else:
            rows[g, k] = z_by_rank[o][g, n] if o == rank else np.float32(0.0)
    return idle2, dead, rows, owner, token


def apply(rows, dead, idle, E, counter, m=None, v=None, vmax=None, ema_n=None, ema_m=None):
    """In place on copies: returns (idle, E, counter = (last, total), dict of the optional arrays).  E and the moments [G, K, D]."""
    idle, E = idle.copy(), E.copy()
    opt = {k: (a.copy() if a is not None else None) for k, a in dict(m=m, v=v, vmax=vmax, ema_n=ema_n, ema_m=ema_m).items()}
    for g, k in zip(*np.nonzero(dead)):
        E[g, k] = rows[g, k]
        for name in ("m", "v", "vmax"):
            if opt[name] is not None:
                opt[name][g, k] = 0.0
        if opt["ema_n"] is not None:
            opt["ema_n"][g, k] = 1.0
        if opt["ema_m"] is not None:
            opt["ema_m"][g, k] = rows[g, k]
        idle[g, k] = 0
    last = int(dead.sum())
    return idle, E, (last, counter[1] + last), opt


def bits(a):
    """The raw words of a float32 array (bitwise comparisons: NaN payloads and the sign of zero count)."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
