"""Two builds of libkvq.so against each other on the LayerNorm family of csrc/kvq_ln.hip: `python tools/ln_compare_libs.py LIB_A
LIB_B`.  Both libraries are loaded into this one process and run on the same seeded inputs; every output is a view inside a frame
of pattern words (bf16 activations: tests/test_ln_parity_gpu.py: _buffer; the other dtypes and the partial rows framed the same
way here) and must be equal BY BITS, its frame included.

  kvq_dropout_residual_ln_fwd            with a residual (pre kept) and without (pre null): out, pre, mean, rstd
  kvq_dropout_residual_ln_bwd_partial    (g_y, g_resid, want_dbias) = (1, 1, 1), (1, 1, 0), (null, 1, 0), (1, null, 1): g_y, g_resid, part
  kvq_ln_dropout_bwd_partial             g_x, part
      H in 64 .. 3072 (every PER of both access widths, H % 8 != 0, the limits; 4096 too for the forward), N in 1, 7, 16, 17, 33
      (part, whole and one-over workgroups of 16 rows and of 4), f32 and bf16, p_drop 0 and 0.1, bf16 also from bases that are
      8-byte but not 16-byte aligned (the 4-wide backward)
  kvq_dropout_residual_ln_bwd            the three gradient destinations adjacent, pairwise adjacent and separate, accumulate 0 / 1,
                                         f32 and bf16 parameter gradients
  kvq_dropout_residual_ln_fwd_fp8        out, pre, mean, rstd, the e4m3 bytes and the words of the delayed-scaling record
  kvq_embed_ln_fwd                       ids below 0 and at V among them
Everything once without and once with a seed offset (kvq_set_seed_offset, set in both libraries).

One line per comparison; the first difference ends the run with exit status 1."""
import ctypes
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_ln_parity_gpu as T  # noqa: E402
from kvq import _ffi  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
KDT = {F32: _ffi.KVQ_F32, BF16: _ffi.KVQ_BF16}
HS = (64, 256, 264, 512, 768, 1024, 1032, 2048, 3072)
NS = (1, 7, 16, 17, 33)
EPS, SEED, SITE = 1e-12, 77, 9
PAT = 0x5A
lines = {}


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _ffi.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def framed(shape, dtype, misaligned=False):
    """(whole allocation, view of `shape` inside it): pattern before and after the payload, which starts 16 bytes (misaligned: 8
    bytes) into the allocation -- T._buffer for bf16 [N, H], the same layout in bytes for everything else"""
    if dtype == BF16 and len(shape) == 2:
        (flat, _), v = T._buffer(shape[0], shape[1], misaligned)
        return flat, v
    n = 1
    for s in shape:
        n *= s
    es = torch.empty(0, dtype=dtype).element_size()
    off = 8 if misaligned else 16
    flat = torch.full((off + n * es + 24,), PAT, dtype=torch.uint8, device="cuda")
    return flat, flat[off:off + n * es].view(dtype).view(*shape)


def filled(src, misaligned=False):
    flat, v = framed(tuple(src.shape), src.dtype, misaligned)
    v.copy_(src)
    return v


def ptr(t):
    return None if t is None else t.data_ptr()


def compare(name, what, run):
    """run(lib) -> {output name: whole framed allocation} under each library in turn"""
    res = []
    for lib in LIBS:
        res.append(run(lib))
    torch.cuda.synchronize()
    a, b = res
    for k in a:
        wa, wb = a[k].view(torch.uint8), b[k].view(torch.uint8)
        if not torch.equal(wa, wb):
            diff = (wa != wb).nonzero()
            sys.exit(f"{name} {what}: DIFFERENT {k}: {len(diff)} of {wa.numel()} bytes, the first at {int(diff[0])}")
    lines[name] = lines.get(name, 0) + 1
    print(f"{name} {what}: equal ({', '.join(f'{k} {a[k].numel()}' for k in a)})")


def call(lib, name, *args):
    rc = getattr(lib, name)(*args)
    if rc != 0:
        msg = lib.kvq_last_error()
        sys.exit(f"{name} failed with code {rc}: {msg.decode() if msg else '?'}")


def rnd(gen, *shape):
    return torch.randn(*shape, device="cuda", generator=gen)


def forward(lib, dt, N, H, p, mis, y, r, gamma, beta, keep_pre, fp8_state=None):
    """-> (outputs by name, pre view, mean view, rstd view)"""
    fo, out = framed((N, H), dt, mis)
    fp, pre = framed((N, H), dt, mis) if keep_pre else (None, None)
    fm, mean = framed((N,), F32)
    fr, rstd = framed((N,), F32)
    res = dict(out=fo, mean=fm, rstd=fr)
    if keep_pre:
        res["pre"] = fp
    st = _ffi.stream_ptr()
    if fp8_state is None:
        call(lib, "kvq_dropout_residual_ln_fwd", ptr(y), ptr(r), ptr(gamma), ptr(beta), N, H, EPS, p, SEED, SITE, KDT[dt], ptr(out), ptr(pre),
             ptr(mean), ptr(rstd), st)
    else:
        f8, out8 = framed((N, H), torch.uint8)
        state = fp8_state.clone()
        call(lib, "kvq_dropout_residual_ln_fwd_fp8", ptr(y), ptr(r), ptr(gamma), ptr(beta), N, H, EPS, p, SEED, SITE, ptr(out), ptr(pre),
             ptr(mean), ptr(rstd), ptr(out8), ptr(state), st)
        res.update(out_fp8=f8, fp8_state=state)
    return res, pre, mean, rstd


def part_buffer(lib, N, H):
    rows = lib.kvq_ln_bwd_partial_rows(N)
    nbytes = lib.kvq_ln_bwd_workspace_bytes(N, H)
    assert nbytes == rows * 3 * H * 4
    flat, part = framed((rows, 3 * H), F32)
    return flat, part, nbytes


def family(dt, N, H, p, mis, tag):
    gen = torch.Generator(device="cuda").manual_seed(H * 10007 + N * 13 + (1 if mis else 0))
    y, r, g = (filled(rnd(gen, N, H).to(dt), mis) for _ in range(3))
    gamma, beta = filled(1 + 0.5 * rnd(gen, H)), filled(0.5 * rnd(gen, H))
    what = f"H = {H}, N = {N}, {str(dt)[6:]}, p = {p}, {'8-byte' if mis else '16-byte'} bases, {tag}"
    compare("kvq_dropout_residual_ln_fwd", what + ", residual", lambda lib: forward(lib, dt, N, H, p, mis, y, r, gamma, beta, True)[0])
    compare("kvq_dropout_residual_ln_fwd", what + ", no residual, pre null", lambda lib: forward(lib, dt, N, H, p, mis, y, None, gamma, beta, False)[0])
    if H > 3072:
        return
    _, pre, mean, rstd = forward(LIBS[0], dt, N, H, p, mis, y, r, gamma, beta, True)
    st = _ffi.stream_ptr()

    def bwd(lib, want_gy, want_gr, want_dbias):
        fy, gy = framed((N, H), dt, mis) if want_gy else (None, None)
        fr, gr = framed((N, H), dt, mis) if want_gr else (None, None)
        fpart, part, nbytes = part_buffer(lib, N, H)
        call(lib, "kvq_dropout_residual_ln_bwd_partial", ptr(g), ptr(pre), ptr(mean), ptr(rstd), ptr(gamma), N, H, p, SEED, SITE, KDT[dt], ptr(gy),
             ptr(gr), want_dbias, ptr(part), nbytes, st)
        return {k: v for k, v in dict(g_y=fy, g_resid=fr, part=fpart).items() if v is not None}

    for want in ((1, 1, 1), (1, 1, 0), (0, 1, 0), (1, 0, 1)):
        compare("kvq_dropout_residual_ln_bwd_partial", what + f", (g_y, g_resid, want_dbias) = {want}", lambda lib: bwd(lib, *want))

    def dbwd(lib):
        fx, gx = framed((N, H), dt, mis)
        fpart, part, nbytes = part_buffer(lib, N, H)
        call(lib, "kvq_ln_dropout_bwd_partial", ptr(g), ptr(pre), ptr(mean), ptr(rstd), ptr(gamma), N, H, p, SEED, SITE, KDT[dt], ptr(gx), ptr(part),
             nbytes, st)
        return dict(g_x=fx, part=fpart)
    compare("kvq_ln_dropout_bwd_partial", what, dbwd)


def full_backward(dt, pdt, N, H, layout, accumulate, tag):
    gen = torch.Generator(device="cuda").manual_seed(H * 7919 + N)
    y, r, g = (filled(rnd(gen, N, H).to(dt)) for _ in range(3))
    gamma, beta = filled(1 + 0.5 * rnd(gen, H)), filled(0.5 * rnd(gen, H))
    _, pre, mean, rstd = forward(LIBS[0], dt, N, H, 0.1, False, y, r, gamma, beta, True)
    start = rnd(gen, 3 * H + 64).to(pdt)
    st = _ffi.stream_ptr()

    def run(lib):
        fy, gy = framed((N, H), dt)
        fr, gr = framed((N, H), dt)
        fg, grads = framed((3 * H + 64,), pdt)               # [dense bias | LN weight | LN bias] with 16 / 32 spare elements between
        grads.copy_(start)
        o = {"adjacent": (0, H, 2 * H), "pairwise": (0, H + 16, 2 * H + 16), "separate": (0, H + 16, 2 * H + 48)}[layout]
        gb, gg, gbt = (grads[i:i + H] for i in o)
        ws = torch.empty(lib.kvq_ln_bwd_workspace_bytes(N, H), dtype=torch.uint8, device="cuda")
        call(lib, "kvq_dropout_residual_ln_bwd", ptr(g), ptr(pre), ptr(mean), ptr(rstd), ptr(gamma), N, H, 0.1, SEED, SITE, KDT[dt], ptr(gy), ptr(gr),
             ptr(gg), ptr(gbt), ptr(gb), KDT[pdt], accumulate, ptr(ws), ws.numel(), st)
        return dict(g_y=fy, g_resid=fr, param_grads=fg)
    compare("kvq_dropout_residual_ln_bwd", f"H = {H}, N = {N}, io {str(dt)[6:]}, gradients {str(pdt)[6:]} {layout}, accumulate {accumulate}, {tag}", run)


def fp8_forward(N, H, p, with_resid, tag):
    gen = torch.Generator(device="cuda").manual_seed(H * 104729 + N)
    y, r = (filled(rnd(gen, N, H).to(BF16)) for _ in range(2))
    gamma, beta = filled(1 + 0.5 * rnd(gen, H)), filled(0.5 * rnd(gen, H))
    state = torch.zeros(LIBS[0].kvq_fp8_state_floats(), device="cuda")
    state[0] = 37.0                                               # the scale of the previous step
    compare("kvq_dropout_residual_ln_fwd_fp8", f"H = {H}, N = {N}, p = {p}, {'residual' if with_resid else 'no residual'}, {tag}",
            lambda lib: forward(lib, BF16, N, H, p, False, y, r if with_resid else None, gamma, beta, True, fp8_state=state)[0])


def embed_forward(dt, N, H, p, tag):
    V, S = 50, 5
    gen = torch.Generator(device="cuda").manual_seed(H * 15485863 + N)
    ids = torch.randint(0, V, (N,), device="cuda", generator=gen)
    ids[0] = -3
    ids[N // 2] = V
    word, pos, type_row = filled(rnd(gen, V, H).to(dt)), filled(rnd(gen, S, H).to(dt)), filled(rnd(gen, 1, H).to(dt))
    gamma, beta = filled(1 + 0.5 * rnd(gen, H)), filled(0.5 * rnd(gen, H))

    def run(lib):
        fo, out = framed((N, H), dt)
        fp, pre = framed((N, H), dt)
        fm, mean = framed((N,), F32)
        fr, rstd = framed((N,), F32)
        call(lib, "kvq_embed_ln_fwd", ptr(ids), ptr(word), ptr(pos), ptr(type_row), ptr(gamma), ptr(beta), N, S, H, V, EPS, p, SEED, SITE, KDT[dt],
             ptr(out), ptr(pre), ptr(mean), ptr(rstd), _ffi.stream_ptr())
        return dict(out=fo, pre=fp, mean=fm, rstd=fr)
    compare("kvq_embed_ln_fwd", f"H = {H}, N = {N}, {str(dt)[6:]}, p = {p}, ids -3 and V, {tag}", run)


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    LIBS = [load(p) for p in sys.argv[1:]]
    counter = torch.tensor([12345], dtype=torch.int64, device="cuda")
    for off, tag in ((None, "no seed offset"), (counter, "seed offset 12345")):
        for lib in LIBS:
            call(lib, "kvq_set_seed_offset", ptr(off))
        for p in (0.0, 0.1):
            for N in NS:
                for H in HS + (4096,):
                    family(F32, N, H, p, False, tag)
                    family(BF16, N, H, p, False, tag)
                    family(BF16, N, H, p, True, tag)
                    fp8_forward(N, H, p, True, tag)
                    fp8_forward(N, H, p, False, tag)
                    embed_forward(F32, N, H, p, tag)
                    embed_forward(BF16, N, H, p, tag)
        for H in HS:
            for N in (7, 33):
                for dt in (F32, BF16):
                    for pdt in (F32, BF16):
                        for layout in ("adjacent", "pairwise", "separate"):
                            for accumulate in (0, 1):
                                full_backward(dt, pdt, N, H, layout, accumulate, tag)
    for lib in LIBS:
        call(lib, "kvq_set_seed_offset", None)
    print(f"{sys.argv[1]} and {sys.argv[2]}: {sum(lines.values())} comparisons, every output equal by bits (" +
          ", ".join(f"{n} {c}" for n, c in lines.items()) + ")")
