"""One bf16 attention forward + backward through libkvq.so with every output inside a framed buffer, in the layouts the engine uses
(tests/test_attn_parity_gpu.py).  Run as a program it is the child of the arms test: it computes the reduced case list ARM_CASES under
whatever KVQ_ATTN_COAL / KVQ_ATTN_STC its environment sets and writes the outputs to the file named by its argument.

Layouts:
  "qkv"    self-attention: q, k, v are the three column thirds of one [N, 3H] buffer, the gradients the thirds of another; the
           k / v bias partials are the halves of one [B, 2H] buffer.
  "cross"  cross-attention as kvq/engine.py::_cakv_batched lays it out: k, v are the two halves of layer `layer`'s 2H columns of a
           [B*Sk, L*2H] buffer, g_k / g_v the same slice of the gradient buffer, the k / v bias partials that slice of [B, L*2H].
`cpad` bf16 / f32 elements of frame stand left and right of every buffer's payload columns (0: the payload is the whole row, as in
the step), `rpad` rows before it and rpad + 1 rows after it.  Every output buffer is filled with a fixed bit pattern first;
run() asserts bit for bit that nothing outside the payload changed.
"""
from __future__ import annotations

import sys

import torch

PAT16 = 0x5A5A                     # bf16 1.5e16: not a value any kernel here produces
PAT32 = 0x5A5A5A5A


class Framed:
    def __init__(self, rows, cols, dtype, rpad, cpad, device="cuda"):
        self.rows, self.cols, self.rpad, self.cpad = rows, cols, rpad, cpad
        self.idt, self.pat = (torch.int16, PAT16) if dtype == torch.bfloat16 else (torch.int32, PAT32)
        self.big = torch.empty((rpad + rows + rpad + 1, cpad + cols + cpad), dtype=dtype, device=device)
        self.big.view(self.idt).fill_(self.pat)
        self.view = self.big[rpad:rpad + rows, cpad:cpad + cols]

    def cols_of(self, c0, c1):
        return self.view[:, c0:c1]

    def assert_frame(self, what, written=None):
        """bitwise: everything outside the payload (or outside the column ranges `written` of the payload rows) is untouched"""
        ok = self.big.view(self.idt) == self.pat
        for c0, c1 in (written if written is not None else [(0, self.cols)]):
            ok[self.rpad:self.rpad + self.rows, self.cpad + c0:self.cpad + c1] = True
        bad = torch.nonzero(~ok)
        assert bad.numel() == 0, f"{what}: {bad.shape[0]} elements outside the output were written, first at (row, column) " \
                                 f"{tuple(int(x) for x in bad[0])} of a buffer with payload rows {self.rpad}..{self.rpad + self.rows}, " \
                                 f"columns {self.cpad}..{self.cpad + self.cols}"


def heads(t, B, S, nh):
    """[B*S, nh*64] view -> [B, nh, S, 64]"""
    return t.reshape(B, S, nh, 64).permute(0, 2, 1, 3).contiguous()


def make_mask(kind, B, Sk, gen):
    """None | "prefix" (lengths in [1, Sk], first sentence full, LAST sentence the shortest) | "holes" (random bits, at least one
    attended key per sentence, some sentences with key 0 masked) | "empty<b>" (prefix, sentence b attends to nothing)"""
    if kind is None:
        return None
    ar = torch.arange(Sk, device="cuda")
    if kind == "holes":
        m = (torch.rand(B, Sk, device="cuda", generator=gen) < 0.6).long()
        m[torch.arange(B, device="cuda"), torch.randint(0, Sk, (B,), device="cuda", generator=gen)] = 1
        m[-1] = 0
        m[-1, Sk // 2] = 1                                # the last sentence is the shortest: one key, and not key 0
        return m
    lens = torch.randint(1, Sk + 1, (B,), device="cuda", generator=gen)
    lens[0] = Sk
    lens[-1] = 1
    m = (ar[None] < lens[:, None]).long()
    if kind.startswith("empty"):
        m[int(kind[5:])] = 0
    return m


def run(B, nh, Sq, Sk, causal, mask_kind, p, layout, seed=1, site=3, cpad=8, rpad=2, L=12, layer=5, partials=True):
    """Returns (inputs, got): inputs = dict(q, k, v, g_out in head layout, mask), got = dict(ctx, lse, g_q, g_k, g_v, pb_q, pb_k,
    pb_v) in head layout (tests/_attn_ref.py)."""
    from kvq import _ffi, nnops
    lib = _ffi.lib()
    bf = torch.bfloat16
    H = nh * 64
    gen = torch.Generator(device="cuda").manual_seed(1000003 * seed + 131 * Sq + Sk)
    rnd = lambda rows, cols: torch.randn(rows, cols, device="cuda", generator=gen).to(bf)
    mask = make_mask(mask_kind, B, Sk, gen)
    frames = []
    if layout == "qkv":
        assert Sq == Sk
        X = Framed(B * Sq, 3 * H, bf, rpad, cpad)
        X.view.copy_(rnd(B * Sq, 3 * H))
        G = Framed(B * Sq, 3 * H, bf, rpad, cpad)
        q, k, v = (X.cols_of(i * H, (i + 1) * H) for i in range(3))
        gq, gk, gv = (G.cols_of(i * H, (i + 1) * H) for i in range(3))
        PK = Framed(B, 2 * H, torch.float32, 1, cpad)
        pbk, pbv = PK.cols_of(0, H), PK.cols_of(H, 2 * H)
        frames += [(G, "g_q | g_k | g_v", None), (PK, "pb_k | pb_v", None)]
        snap = [(X.big, X.big.clone())]
    else:
        XQ = Framed(B * Sq, H, bf, rpad, cpad)
        XQ.view.copy_(rnd(B * Sq, H))
        GQ = Framed(B * Sq, H, bf, rpad, cpad)
        KV = Framed(B * Sk, L * 2 * H, bf, rpad, 0)
        KV.view.copy_(rnd(B * Sk, L * 2 * H))
        GKV = Framed(B * Sk, L * 2 * H, bf, rpad, 0)
        c0 = layer * 2 * H
        q, gq = XQ.view, GQ.view
        k, v = KV.cols_of(c0, c0 + H), KV.cols_of(c0 + H, c0 + 2 * H)
        gk, gv = GKV.cols_of(c0, c0 + H), GKV.cols_of(c0 + H, c0 + 2 * H)
        PK = Framed(B, L * 2 * H, torch.float32, 1, 0)
        pbk, pbv = PK.cols_of(c0, c0 + H), PK.cols_of(c0 + H, c0 + 2 * H)
        frames += [(GQ, "g_q", None), (GKV, "g_k | g_v", [(c0, c0 + 2 * H)]), (PK, "pb_k | pb_v", [(c0, c0 + 2 * H)])]
        snap = [(XQ.big, XQ.big.clone()), (KV.big, KV.big.clone())]
    PQ = Framed(B, H, torch.float32, 1, cpad)
    CTX = Framed(B * Sq, H, bf, rpad, cpad)
    GO = Framed(B * Sq, H, bf, rpad, cpad)
    GO.view.copy_(rnd(B * Sq, H))
    LSE = torch.empty(4 + B * nh * Sq + 5, dtype=torch.float32, device="cuda")
    LSE.view(torch.int32).fill_(PAT32)
    lse = LSE[4:4 + B * nh * Sq].view(B, nh, Sq)
    frames += [(PQ, "pb_q", None), (CTX, "ctx", None)]
    snap.append((GO.big, GO.big.clone()))
    ctx, g = CTX.view, GO.view
    _ffi.check(lib.kvq_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), None if mask is None else mask.data_ptr(), B, nh, Sq, Sk, 64,
                                q.stride(0), k.stride(0), v.stride(0), ctx.stride(0), int(causal), 0.125, float(p), seed, site,
                                _ffi.KVQ_BF16, ctx.data_ptr(), lse.data_ptr(), _ffi.stream_ptr()), "kvq_attn_fwd")
    long = Sq > 32 or Sk > 32
    pb = (PQ.view, pbk, pbv) if partials else (None, None, None)
    nnops.attn_bwd(q, k, v, mask, g, B, nh, Sq, Sk, causal, p, seed, site, gq, gk, gv, *pb,
                   ctx=ctx if long else None, lse=lse if long else None)
    torch.cuda.synchronize()
    for f, what, written in frames:
        f.assert_frame(what, written if partials or not what.startswith("pb_") else [])     # no partials asked: all pattern
    ok = LSE.view(torch.int32) == PAT32
    assert bool(ok[:4].all()) and bool(ok[4 + B * nh * Sq:].all()), "lse: written outside [B, nh, Sq]"
    for big, before in snap:
        assert torch.equal(big.view(torch.int16), before.view(torch.int16)), "an input buffer was written"
    inputs = dict(q=heads(q, B, Sq, nh), k=heads(k, B, Sk, nh), v=heads(v, B, Sk, nh), g_out=heads(g, B, Sq, nh), mask=mask)
    got = dict(ctx=heads(ctx, B, Sq, nh), lse=lse.clone(), g_q=heads(gq, B, Sq, nh), g_k=heads(gk, B, Sk, nh), g_v=heads(gv, B, Sk, nh))
    if partials:
        got.update(pb_q=PQ.view.reshape(B, nh, 64).clone(), pb_k=pbk.reshape(B, nh, 64).clone(), pb_v=pbv.reshape(B, nh, 64).clone())
    return inputs, got


def reveal_keep(B, nh, Sq, Sk, p, seed=1, site=3):
    """The keep mask [B, nh, Sq, Sk] the kernels draw for (seed, site): q = k = 0 makes the probabilities uniform, one-hot V rows
    carry P~[i][j] = keep / (Sk (1 - p)) to column j of the output -- 64 keys per pass.  The Philox bits are indexed by
    (sentence * nh + head, query, key) alone (attn_keep16() / blk_keep16() in csrc/kvq_nn.hip: ((bh * SQP + i) * SKP + j) >> 2 with
    SQP = SKP = 32, resp. Sq / Sk rounded up to 32), so the mask does not depend on values, mask, causal or row strides."""
    from kvq import nnops
    H = nh * 64
    z = torch.zeros(B * Sq, H, device="cuda", dtype=torch.bfloat16)
    zk = torch.zeros(B * Sk, H, device="cuda", dtype=torch.bfloat16)
    keep = torch.empty(B, nh, Sq, Sk, device="cuda", dtype=torch.float64)
    for j0 in range(0, Sk, 64):
        n = min(64, Sk - j0)
        eye = torch.zeros(Sk, 64, device="cuda")
        eye[torch.arange(j0, j0 + n), torch.arange(n)] = 1
        v1 = eye[None, :, None, :].expand(B, Sk, nh, 64).reshape(B * Sk, H).contiguous().bfloat16()
        ctx, _ = nnops.attn_fwd(z, zk, v1, None, B, nh, Sq, Sk, False, p, seed=seed, site=site)
        keep[..., j0:j0 + n] = (heads(ctx, B, Sq, nh)[..., :n] > 0).double()
    return keep


# the arms test's reduced list: one step-shape case with dropout, one ragged cross-attention case
ARM_CASES = {
    "step": dict(B=256, nh=12, Sq=32, Sk=32, causal=True, mask_kind="prefix", p=0.1, layout="qkv", cpad=0),
    "cross": dict(B=5, nh=12, Sq=9, Sk=12, causal=False, mask_kind="holes", p=0.1, layout="cross"),
}


def main(path):
    out = {}
    for name, kw in ARM_CASES.items():                  # any failure raises: the process ends there with a non-zero status
        _, got = run(**kw)
        out[name] = {k: t.cpu() for k, t in got.items()}
    torch.save(out, path)


if __name__ == "__main__":
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    for d in (os.path.join(root, "kindergarten-vq-vae_amd"), here):
        if d not in sys.path:
            sys.path.insert(0, d)
    main(sys.argv[1])
