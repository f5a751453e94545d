"""Bit-exact parity of the bf16 GEMM family (csrc/kvq_gemm2.hip, csrc/kvq_gemm_any.hip, the router kvq.nnops.gemm) against an f64
matmul on the CPU, and per-element parity of the fused GELU / GELU' / softmax-statistics epilogues.

Operands are integers in [-8, 8] without 0 times a power of two, inside the range where every f32 partial sum of any grouping is
exact (tests/_gemm_ref.py: assert_gemm_exact_range, called before every launch): the stored value must be bf16_rne(A.B + bias)
bit for bit -- with accumulate bf16_rne(bf16_rne(A.B + bias) + C_old).  Every output sits in a canary frame whose bits must not
change.  Shapes are the smallest that reach an arm of the kernels:
  k-tiles 1 .. 7 against rings of 2 and 3 slots (nkt < NPRO, the EARLY prologue, wrap-around): test_core K = 64 .. 448
  9 tiles, ntiles % 8 != 0 (XCD renumbering with a remainder): test_core (2BM+8, 2BN+8)
  column bands of 6 tile columns with a narrower last band (band = -6, mg_rem): test_core (BM+8, 7BN+8) and N = 12*128+8 on 64x128
  the multi-problem kernel's tile look-up on every layout: test_grouped_*, test_mixed_tile_launch
  the persistent tile loop with one and two tiles per workgroup: test_persistent
Every test judges every element.  Measured figures and the arm-by-arm list of test ids: profiles/gemm_exact_parity.md."""
import functools

import pytest
import torch

import _gemm_ref as G
import _pointwise_ref as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
TILE_DIMS = {"128x192": (128, 192), "128x256": (128, 256), "256x192": (256, 192), "256x256": (256, 256), "64x128": (64, 128),
             "128x192h": (128, 192)}
CANARY = 77.0


@pytest.fixture(scope="module")
def ops():
    from kvq import _ffi, nnops
    _ffi.lib()
    assert torch.cuda.is_available()
    return nnops


@functools.lru_cache(maxsize=None)
def _case(layout, M, N, K, seed, bias=False, accumulate=False, padded=False, ea=0, eb=0, ebias=None):
    """A case, checked to be inside the exact range, and the f64 value whose RNE rounding must be stored (never modified)."""
    c = G.make_case(layout, M, N, K, seed, bias=bias, accumulate=accumulate, padded=padded, ea=ea, eb=eb, ebias=ebias)
    G.case_exact_range(c)
    return c, G.case_ref(c)[1]


def _framed(M, N, c_old=None):
    """(frame, out): out [M, N] one row and eight columns inside a frame of CANARY, holding the old C when there is one."""
    frame = torch.full((M + 2, N + 16), CANARY, dtype=BF16, device="cuda")
    out = frame[1:M + 1, 8:8 + N]
    if c_old is not None:
        out.copy_(c_old)
    return frame, out


def _frame_intact(frame, M, N):
    f = frame.cpu().float()
    return bool((f[0] == CANARY).all() and (f[M + 1] == CANARY).all() and (f[:, :8] == CANARY).all() and (f[:, 8 + N:] == CANARY).all())


def _mfma_gemm(ops, c, tile, what):
    """nnops.gemm on the MFMA route into a canary frame; the output on the CPU."""
    a, b = G.on_device(c.a), G.on_device(c.b)
    bias = c.bias.cuda() if c.bias is not None else None
    frame, out = _framed(c.M, c.N, c.c_old)
    before = dict(ops.GEMM_ROUTES)
    ops.gemm(a, b, c.layout, bias=bias, out=out, accumulate=c.c_old is not None, tile=tile)
    moved = {k: v - before[k] for k, v in ops.GEMM_ROUTES.items() if v != before[k]}
    assert moved == {"mfma": 1}, f"{what}: routed {moved}"
    assert _frame_intact(frame, c.M, c.N), f"{what}: wrote outside its output"
    return out.cpu()


def _core_shapes(tile):
    bm, bn = TILE_DIMS[tile]
    s = [(8, 8, 64)] + [(bm + 8, bn + 8, K) for K in (64, 128, 192, 256, 448)] + [(2 * bm + 8, 2 * bn + 8, 128), (bm + 8, 7 * bn + 8, 64)]
    if tile == "64x128":
        s.append((bm + 8, 12 * bn + 8, 64))
    return s


CORE = [(t, s) for t in TILE_DIMS for s in _core_shapes(t)]


@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("tile,shape", CORE, ids=[f"{t}-{m}x{n}x{k}" for t, (m, n, k) in CORE])
def test_core(ops, layout, tile, shape):
    M, N, K = shape
    c, final = _case(layout, M, N, K, seed=M + 3 * N + 5 * K)
    what = f"{tile} {layout} {shape}"
    G.assert_exact(_mfma_gemm(ops, c, tile, what), final, what)


@pytest.mark.parametrize("variant", ["bias", "accumulate", "strided", "all"])
@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("tile", list(TILE_DIMS))
def test_bias_accumulate_strides(ops, tile, layout, variant):
    """N = BN + 8: the last 16-column block of the second tile column is half outside (the bias clamp nb + 4 <= N)."""
    bm, bn = TILE_DIMS[tile]
    M, N, K = bm + 8, bn + 8, 192
    c, final = _case(layout, M, N, K, seed=M + N + 11, bias=variant in ("bias", "all"), accumulate=variant in ("accumulate", "all"),
                     padded=variant in ("strided", "all"))
    if c.a.stride(0) != c.a.shape[1]:
        assert c.a.stride(0) == c.a.shape[1] + G.PAD_LD and c.b.stride(0) == c.b.shape[1] + G.PAD_LD
    what = f"{tile} {layout} {variant}"
    G.assert_exact(_mfma_gemm(ops, c, tile, what), final, what)


# ---------------------------------------------------------------------------------------------------------------
# several problems per launch
# ---------------------------------------------------------------------------------------------------------------
def _grouped(ops, specs, launch):
    """specs: (case, final) per problem.  launch(problems) runs them; every problem is judged against its own reference."""
    keep, probs = [], []
    for c, final in specs:
        a, b = G.on_device(c.a), G.on_device(c.b)
        bias = c.bias.cuda() if c.bias is not None else None
        frame, out = _framed(c.M, c.N, c.c_old)
        probs.append(ops.gemm_problem(a, b, out, c.layout, bias=bias, accumulate=c.c_old is not None))
        keep.append((a, b, bias, frame, out))
    launch(probs)
    torch.cuda.synchronize()
    for i, ((c, final), (_, _, _, frame, out)) in enumerate(zip(specs, keep)):
        what = f"problem {i} ({c.layout} {c.M} x {c.N} x {c.K})"
        assert _frame_intact(frame, c.M, c.N), f"{what}: wrote outside its output"
        G.assert_exact(out.cpu(), final, what)


@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("tile", ["128x256", "64x128"])
def test_grouped_three_problems(ops, tile, layout):
    """gemm2_kernel (the non-SINGLE locate_tile) on every layout: 4 + 3 + 3 tiles, different M, N, K, a bias, an accumulate."""
    bm, bn = TILE_DIMS[tile]
    specs = [_case(layout, bm + 8, bn + 8, 128, seed=101, bias=True),
             _case(layout, 8, 2 * bn + 8, 64, seed=102, accumulate=True),
             _case(layout, 2 * bm + 8, 8, 192, seed=103, padded=True)]
    _grouped(ops, specs, lambda p: ops.gemm_grouped(p, layout, tile))


def test_grouped_sixteen_tiny_problems(ops):
    specs = [_case("tn", 8 * (i + 1), 8 * (16 - i), 64 * (1 + i % 3), seed=200 + i, bias=i % 4 == 1, accumulate=i % 4 == 2) for i in range(16)]
    _grouped(ops, specs, lambda p: ops.gemm_grouped(p, "tn", "256x256"))


@pytest.mark.parametrize("tiles", [("256x256", "128x256"), ("128x256", "256x256"), ("256x256",), ("128x256",)])
def test_mixed_tile_launch(ops, tiles):
    """gemm2_mixed_kernel: two tile classes in one grid (either order of the caller's list), and each class alone."""
    shapes = [(264, 264), (136, 520)]
    specs = [_case("tn", m, n, 128, seed=300 + i, bias=i == 1) for i, (m, n) in enumerate(shapes[:len(tiles)])]
    _grouped(ops, specs, lambda p: ops.gemm_grouped_mixed(p, list(tiles), "tn"))


# ---------------------------------------------------------------------------------------------------------------
# persistent tile loop
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", ["128x192", "128x256", "256x192", "256x256"])
def test_persistent(ops, tile):
    """KVQ_GEMM_PERSISTENT (nt): a ragged shape of 4 tiles, and one whose tile count lies strictly between one and two times the CU
    count (some workgroups walk two tiles, the others one); K = 192 and 256 (K = 192: the first 192 columns of the K = 256
    operands, row stride 256), with and without bias."""
    bm, bn = TILE_DIMS[tile]
    cus = ops.cu_count(torch.device("cuda", 0))
    rows = (cus + cus // 4) // 2 + 1                       # 2 tile columns: 1.25 cus + 2 tiles
    for M, N in ((bm + 8, bn + 8), ((rows - 1) * bm + 8, bn + 8)):
        ntiles = -(-M // bm) * -(-N // bn)
        assert ntiles == 4 or cus < ntiles < 2 * cus
        c = G.make_case("nt", M, N, 256, seed=M + N + 13, bias=True)
        G.case_exact_range(c)                              # covers K = 192 too: S only grows with K
        a, b, bias = c.a.cuda(), c.b.cuda(), c.bias.cuda()
        for K in (192, 256):
            y = c.A[:, :K] @ c.B[:K]
            for bv in (bias, None):
                final = y + c.bias.double()[None, :] if bv is not None else y
                frame, out = _framed(M, N)
                before = ops.GEMM_ROUTES["mfma"]
                ops.gemm(a[:, :K], b[:, :K], "nt", bias=bv, out=out, tile=tile + "p")
                assert ops.GEMM_ROUTES["mfma"] == before + 1
                what = f"{tile}p {M} x {N} x {K} ({ntiles} tiles, {cus} CUs) bias={bv is not None}"
                assert _frame_intact(frame, M, N), f"{what}: wrote outside its output"
                G.assert_exact(out.cpu(), final, what)


# ---------------------------------------------------------------------------------------------------------------
# any-shape kernel and the router
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("shape", [(7, 5, 3), (72, 9, 128), (333, 130, 129)])
def test_any_shape_kernel(ops, layout, shape):
    from kvq._ffi import check, lib, stream_ptr
    M, N, K = shape
    code = {"nt": 0, "nn": 1, "tn": 2}[layout]
    for bias, accumulate in ((True, False), (False, True), (True, True)):
        c, final = _case(layout, M, N, K, seed=M + N + K + 17, bias=bias, accumulate=accumulate)
        a, b = c.a.cuda(), c.b.cuda()
        bv = c.bias.cuda() if bias else None
        frame, out = _framed(M, N, c.c_old)
        check(lib().kvq_gemm_any_bf16(a.data_ptr(), b.data_ptr(), bv.data_ptr() if bias else None, out.data_ptr(), M, N, K, a.stride(0),
                                      b.stride(0), out.stride(0), code, int(accumulate), stream_ptr()), "kvq_gemm_any_bf16")
        what = f"any-shape {layout} {shape} bias={bias} accumulate={accumulate}"
        assert _frame_intact(frame, M, N), f"{what}: wrote outside its output"
        G.assert_exact(out.cpu(), final, what)


@pytest.mark.parametrize("route,layout,shape,moved", [("tn_padded", "tn", (72, 40, 200), {"tn_padded": 1, "mfma": 1}),
                                                      ("row_split", "nt", (77, 40, 128), {"row_split": 1, "mfma": 1, "any": 1})])
def test_router(ops, route, layout, shape, moved):
    """nnops.gemm: a tn contraction over 200 tokens is zero-padded to 256 for the MFMA kernel; an nt product of 77 rows runs 72 of
    them there and 5 on the any-shape kernel.  With bias and accumulate, exact."""
    M, N, K = shape
    c, final = _case(layout, M, N, K, seed=400 + M, bias=True, accumulate=True)
    frame, out = _framed(M, N, c.c_old)
    before = dict(ops.GEMM_ROUTES)
    ops.gemm(c.a.cuda(), c.b.cuda(), layout, bias=c.bias.cuda(), out=out, accumulate=True)
    assert {k: v - before[k] for k, v in ops.GEMM_ROUTES.items() if v != before[k]} == moved
    assert _frame_intact(frame, M, N), f"{route}: wrote outside its output"
    G.assert_exact(out.cpu(), final, route)


# ---------------------------------------------------------------------------------------------------------------
# fused epilogues
# ---------------------------------------------------------------------------------------------------------------
def _scaled_case(layout, M, N, K, seed, target, bias=True):
    """Operands scaled by a power of two, chosen on the CPU, so that max |A.B + bias| is about `target`; bias 32 quanta coarse."""
    c0, y0 = _case(layout, M, N, K, seed, bias=bias, ebias=5)
    e = G.pick_exponent(y0, target)
    return e, (layout, M, N, K, seed, bias, False, False, e // 2, e - e // 2, e + 5)


def _report(name, ratio):
    i = int(ratio.argmax())
    r, k = divmod(i, ratio.shape[1])
    print(f"FIGURE {name}: worst ratio {float(ratio.reshape(-1)[i]):.4f} at ({r}, {k})")
    return float(ratio.reshape(-1)[i])


@pytest.mark.parametrize("tile", ["256x192", "128x256", "256x192p", "128x256p"])
def test_gelu_epilogue(ops, tile):
    """kvq_gemm_bf16_gelu: Hout = bf16_rne(x W^T + b) exactly, Aout = gelu(Hout) inside the bf16 forward envelope, per element."""
    bm, bn = TILE_DIMS[tile.rstrip("p")]
    M, N, K = bm + 8, bn + 8, 192
    e, key = _scaled_case("nt", M, N, K, 500 + bm, 6.0)
    c, final = _case(*key)
    assert 4.0 <= float(final.abs().max()) <= 9.0 and float(final.std()) > 1.0, "h does not spread over about +-6"
    h, a = ops.gemm_gelu(G.on_device(c.a), G.on_device(c.b), c.bias.cuda(), tile=tile)
    h, a = h.cpu(), a.cpu()
    G.assert_exact(h, final, f"gelu epilogue {tile}: Hout")
    ratio = G.gelu_epilogue_ratio(a, h)
    worst = _report(f"gemm gelu epilogue {tile} (2^{e})", ratio)
    over = (ratio > 1.0).nonzero()[:5].tolist()
    assert worst <= 1.0, f"{int((ratio > 1.0).sum())} elements outside the envelope; first (row, col, h, got): " \
                         f"{[(r, k, float(h[r, k]), float(a[r, k])) for r, k in over]}"


@pytest.mark.parametrize("tile", ["256x192", "128x256"])
def test_dgelu_epilogue(ops, tile):
    """kvq_gemm_bf16_dgelu: out = bf16(g gelu'(h)) with g = bf16_rne(gy W) known exactly, h every finite bf16 value of |h| <= 8;
    part: one row per row tile, the f32 column sum of the STORED out over that tile, within (BM - 1) 2^-24 sum|out|."""
    from kvq._ffi import lib
    bm, bn = TILE_DIMS[tile]
    M, N, K = 2 * bm + 8, bn + 8, 128
    c, final = _case("nn", M, N, K, seed=600 + bm)
    g = G.rne_bf16(final)
    h = G.all_h_values(M, N, seed=601 + bm)
    out, part = ops.gemm_dgelu(G.on_device(c.a), G.on_device(c.b), h.cuda(), tile=tile)
    out, part = out.cpu(), part.cpu()
    ratio = G.dgelu_epilogue_ratio(out, g, h)
    worst = _report(f"gemm dgelu epilogue {tile}", ratio)
    over = (ratio > 1.0).nonzero()[:5].tolist()
    assert worst <= 1.0, f"{int((ratio > 1.0).sum())} elements outside the envelope; first (row, col, g, h, got): " \
                         f"{[(r, k, float(g[r, k]), float(h[r, k]), float(out[r, k])) for r, k in over]}"
    rows = lib().kvq_gemm_dgelu_partial_rows(M, ops.TILES[tile])
    assert rows == 3 and tuple(part.shape) == (rows, N)
    pw = G.dgelu_part_check(part, out, bm)
    print(f"FIGURE gemm dgelu partial rows {tile}: worst error / bound {pw:.4f}")
    assert pw <= 1.0, "a partial row is not the f32 column sum of the stored values of its row tile"


def _duplicate_columns(c, dst, src):
    """Columns dst of the product become copies of columns src (weights and bias): tied logits."""
    c.B[:, dst] = c.B[:, src]
    c.b[dst] = c.b[src]                                   # nt: b is [N, K]
    c.bias[dst] = c.bias[src]


@pytest.mark.parametrize("M,N,V,K", [(296, 776, 770, 128), (264, 520, 510, 64)])
def test_ce_epilogue(ops, M, N, V, K):
    """kvq_gemm_bf16_ce: the logits exactly, and per (row, 256-column tile) the softmax statistics of the STORED logits below V:
    the maximum by value, the FIRST arg-max bit for bit (tied maxima are planted: columns 128..255 repeat 0..127, 260..263
    repeat 256..259 and 272..287 repeat 256..271 -- ties across wave columns, across the four lanes of a row and inside a lane),
    m + log(sum) within 2^-20 max(1, |lse|, max|x|).  Padding columns carry a bias of +50 and take no part; in the second shape
    the last tile lies wholly beyond V and must read (-inf, 0, INT_MAX)."""
    e, key = _scaled_case("nt", M, N, K, 700 + M, 8.0)
    c = G.make_case(*key[:5], bias=True, ea=key[8], eb=key[9], ebias=key[10])
    _duplicate_columns(c, slice(128, 256), slice(0, 128))
    _duplicate_columns(c, slice(260, 264), slice(256, 260))
    _duplicate_columns(c, slice(272, 288), slice(256, 272))
    c.bias[V:] = 50.0
    G.case_exact_range(c)
    final = G.case_ref(c)[1]
    assert 4.0 <= float(final[:, :V].abs().max()) <= 12.0
    logits, stats = ops.gemm_ce(G.on_device(c.a), G.on_device(c.b), c.bias.cuda(), V)
    logits, stats = logits.cpu(), stats.cpu()
    G.assert_exact(logits, final, f"ce epilogue {M} x {N}: logits")
    tiles = (N + 255) // 256
    assert tuple(stats.shape) == (M, tiles, 4) and (tiles * 256 - 256 >= V) == (V == 510)
    res = G.ce_stats_judge(stats, logits, V)
    x = logits.float()[:, :256]
    tied = int(((x == x.max(dim=1, keepdim=True).values).sum(1) > 1).sum())
    assert tied >= M // 2, "the case holds no tied maxima"
    worst = _report(f"gemm ce epilogue {M}x{N} V={V} (2^{e}) lse per tile", res["ratio"])
    assert (res["max_bad"], res["arg_bad"], res["pad_bad"]) == (0, 0, 0), res
    assert worst <= 1.0
