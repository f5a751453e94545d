"""numpy restatement of the weight-EMA kernels (csrc/kvq_weight_ema.hip, include/kvq.h "exponential moving average of the trained
weights"): the same f64 operations in the same order, each rounded on its own, one final rounding to f32.

    decay_at(t, decay)            d = min((double)(float) decay, (1.0 + t) / (10.0 + t))
    update(p, ema, t, decay)      t == 0: a copy of p (ema is not read);  else (float)(d * (double) ema + (1.0 - d) * (double) p)
    advance(state, decay)         (updates, last_decay) -> (updates + 1, t == 0 ? 0 : (float) d)
    swap(p, ema, shadow)          (ema, p, bf16 bits of the new p | None)
skip=True (the gradient guard's flag) returns what came in.  IEEE 754 fixes neither the sign nor the payload of a NaN that an
operation produces, and the host and the device differ there: same_bits() compares bit patterns and lets a NaN match any NaN."""
import numpy as np


def decay_at(t, decay):
    d = np.float64(np.float32(decay))                     # the entry point takes a float
    w = (np.float64(1.0) + np.float64(int(t))) / (np.float64(10.0) + np.float64(int(t)))
    return d if d < w else w


def update(p, ema, t, decay, skip=False):
    """The average behind kvq_weight_ema_update (a new f32 array).  ema may be None when t == 0: it is not read."""
    p = np.asarray(p, dtype=np.float32)
    if skip:
        return np.array(ema, dtype=np.float32, copy=True)
    if int(t) == 0:
        return p.copy()
    d = decay_at(t, decay)
    omd = np.float64(1.0) - d
    with np.errstate(all="ignore"):
        a = d * np.asarray(ema, dtype=np.float32).astype(np.float64)
        b = omd * p.astype(np.float64)
        return (a + b).astype(np.float32)


def advance(state, decay, skip=False):
    """state = (updates, last_decay as a Python float holding an f32 value) behind kvq_weight_ema_advance."""
    t, last = int(state[0]), float(state[1])
    if skip:
        return t, last
    return t + 1, 0.0 if t == 0 else float(np.float32(decay_at(t, decay)))


def bf16_bits(x):
    """f32 -> bf16, round to nearest even, as uint16 bit patterns; a NaN becomes the quiet NaN 0x7fc0 (see same_bits_bf16)."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    r[np.isnan(np.asarray(x, dtype=np.float32))] = 0x7FC0
    return r


def swap(p, ema, shadow=False):
    p, ema = np.asarray(p, dtype=np.float32), np.asarray(ema, dtype=np.float32)
    return ema.copy(), p.copy(), (bf16_bits(ema) if shadow else None)


def same_bits(got, want):
    """Indices where two f32 arrays differ in their bits, a NaN matching any NaN."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    differ = got.view(np.uint32) != want.view(np.uint32)
    differ &= ~(np.isnan(got) & np.isnan(want))
    return np.flatnonzero(differ)


def same_bits_bf16(got, want):
    """The same for uint16 bf16 bit patterns."""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    nan = lambda b: (b & 0x7FFF) > 0x7F80
    return np.flatnonzero((got != want) & ~(nan(got) & nan(want)))
