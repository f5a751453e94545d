"""fp8 input-gradient GEMMs (TrainEngine(fp8_backward=True), off by default): gx = gy . W as the NT product of gy in OCP e5m2 and the
byte-transposed e4m3 weight mirror.  The e5m2 quantisation passes against torch's float8_e5m2 conversion, the byte transpose against
.t(), the mixed-format GEMM against an f32 matmul of the dequantised operands, and the engine: the calibration step, the gradients
against the bf16 backward on identical forward bits, graph replay against eager launches, the refusals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

E5M2_MAX = 57344.0


def _state(scale):
    from kvq._ffi import lib
    st = torch.zeros(lib().kvq_fp8_state_floats(), dtype=torch.float32, device="cuda")
    st[0] = scale
    return st


# ---- 1. quantisation ---------------------------------------------------------------------------------------------------------------
def test_e5m2_quantisation_equals_torch_float8_conversion():
    from kvq import nnops
    torch.manual_seed(0)
    big = (torch.randn(300, 520, device="cuda") * 3e-4).to(torch.bfloat16)          # gradient-sized values
    x = big[:, 8:8 + 504]                                                           # row stride 520, 16-byte aligned start
    q, scale = nnops.fp8_quantize(x, fmt="e5m2")
    s = (E5M2_MAX / x.float().abs().max()).item()
    np.testing.assert_allclose(scale.item(), s, rtol=1e-6)
    want = (x.float() * scale).clamp(-E5M2_MAX, E5M2_MAX).cpu().to(torch.float8_e5m2)
    assert torch.equal(q.cpu(), want.view(torch.uint8))                             # bytes
    assert q.cpu().view(torch.float8_e5m2).float().abs().max().item() == E5M2_MAX   # the largest element lands on the largest e5m2 value
    # e4m3 through the format-taking entry: the bytes and the scale of kvq_fp8_quantize
    q4, s4 = nnops.fp8_quantize(x, fmt="e4m3")
    q0, s0 = nnops.fp8_quantize(x)
    assert torch.equal(q4, q0) and torch.equal(s4, s0)


@pytest.mark.parametrize("cols,ld", [(512, 512), (504, 520), (496, 512)])           # 16 per thread dense / 8 per thread / 16 per thread strided
@pytest.mark.parametrize("fmt,fmax,tdt", [("e5m2", E5M2_MAX, torch.float8_e5m2), ("e4m3", 448.0, torch.float8_e4m3fn)])
def test_delayed_pass_quantises_with_the_records_scale_and_notes_the_amax(cols, ld, fmt, fmax, tdt):
    """kvq_fp8_quantize_delayed_fmt + kvq_fp8_update_scales_fmt: the bytes are torch's conversion of x * scale (saturating: the scale
    is chosen so that a part of the tensor lies beyond the format's range), the next scale is max(fmt) / (4 amax); the amax-only form
    writes nothing and leaves the same amax."""
    from kvq import nnops
    from kvq._ffi import check, lib, stream_ptr
    g = torch.Generator(device="cuda").manual_seed(cols)
    x = (torch.randn((300, ld), generator=g, device="cuda") * 2e-3).to(torch.bfloat16)[:, :cols]
    scale = fmax / 4e-3                                                             # values beyond 2 sigma saturate
    st = _state(scale)
    q = nnops.fp8_quantize_delayed(x, st, fmt)
    want = (x.float() * scale).clamp(-fmax, fmax).cpu().to(tdt)
    assert torch.equal(q.cpu(), want.view(torch.uint8))
    assert q.cpu().view(tdt).float().abs().max().item() == fmax
    st2 = _state(scale)
    assert nnops.fp8_quantize_delayed(x, st2, fmt, amax_only=True) is None
    amax = x.float().abs().max().item()
    assert st[8:].max().item() == amax and st2[8:].max().item() == amax
    for s_ in (st, st2):
        check(lib().kvq_fp8_update_scales_fmt(s_.data_ptr(), 1, 4.0, nnops.FP8_FORMATS[fmt], stream_ptr()), "update")
        np.testing.assert_allclose(s_[0].item(), fmax / (4.0 * amax), rtol=1e-6)
        assert float(s_[8:].abs().max()) == 0.0                                     # partials cleared
    zero = _state(0.0)                                                              # a record that saw nothing keeps its scale
    check(lib().kvq_fp8_update_scales_fmt(zero.data_ptr(), 1, 4.0, nnops.FP8_FORMATS[fmt], stream_ptr()), "update")
    assert zero[0].item() == 0.0


# ---- 2. transpose ------------------------------------------------------------------------------------------------------------------
def _bytes(rows, cols, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (rows, cols), generator=g, device="cuda", dtype=torch.int32).to(torch.uint8)


@pytest.mark.parametrize("rows,cols,ld", [(16, 16, 16), (128, 128, 128), (2304, 768, 768), (784, 272, 304),
                                          (16, 2064, 2064), (2064, 16, 16)])     # one tile row / column of 17 tiles, every one an edge tile
def test_transpose_is_bitwise(rows, cols, ld):
    from kvq import nnops
    buf = _bytes(rows, ld, rows + cols)
    x8 = buf[:, ld - cols:] if ld != cols else buf                                  # (784, 272): a view with a larger row stride
    assert x8.stride(0) == ld and x8.data_ptr() % 16 == 0
    out = nnops.fp8_transpose(x8)
    assert out.shape == (cols, rows) and torch.equal(out, x8.t().contiguous())
    wide = torch.full((cols, rows + 32), 0xAB, dtype=torch.uint8, device="cuda")    # a destination with a larger row stride: nothing beside it
    nnops.fp8_transpose(x8, out=wide[:, 16:16 + rows])
    assert torch.equal(wide[:, 16:16 + rows], x8.t()) and bool((wide[:, :16] == 0xAB).all()) and bool((wide[:, 16 + rows:] == 0xAB).all())


def test_segmented_transpose_equals_the_single_calls():
    from kvq import nnops
    shapes = [(2304, 768), (16, 16), (128, 128)]
    mats = [_bytes(r, c, 7 + i) for i, (r, c) in enumerate(shapes)]
    src = torch.cat([m.reshape(-1) for m in mats] + [torch.zeros(64, dtype=torch.uint8, device="cuda")])
    dst = torch.full((src.numel() + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    offs = np.cumsum([0] + [r * c for r, c in shapes])[:-1].tolist()
    doffs = [o + 32 for o in offs]                                                  # another layout on the destination side
    t64 = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda")
    tiles = max(-(-r // 128) * -(-c // 128) for r, c in shapes)
    nnops.fp8_transpose_segments(src, dst, t64(offs), t64([r for r, _ in shapes]), t64([c for _, c in shapes]), t64(doffs), tiles)
    for m, (r, c), d in zip(mats, shapes, doffs):
        assert torch.equal(dst[d:d + r * c].view(c, r), nnops.fp8_transpose(m))
    assert bool((dst[:32] == 0xCD).all()) and bool((dst[doffs[-1] + 128 * 128:] == 0xCD).all())


# ---- 3. the mixed-format GEMM --------------------------------------------------------------------------------------------------------
def _operands(M, N, K, w_scale=0.05, x_scale=1.0):
    from kvq import nnops
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    x = (torch.randn((M, K), generator=g, device="cuda") * x_scale).to(torch.bfloat16)
    w = (torch.randn((N, K), generator=g, device="cuda") * w_scale).to(torch.bfloat16)
    bias = torch.randn(N, generator=g, device="cuda").to(torch.bfloat16)
    x8, sx = nnops.fp8_quantize(x, fmt="e5m2")
    w8, sw = nnops.fp8_quantize(w)
    xf = x8.cpu().view(torch.float8_e5m2).float().cuda()
    wf = w8.cpu().view(torch.float8_e4m3fn).float().cuda()
    return x, w, bias, x8, sx, w8, sw, (xf @ wf.t()) / (sx * sw)


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("shape", [(512, 768, 256), (40, 24, 128), (1000, 776, 384), (264, 768, 2304)])
def test_mixed_format_gemm_equals_f32_matmul_of_the_dequantised_operands(shape, with_bias):
    """A in e5m2, B in e4m3.  Products of a 3-bit and a 4-bit significand are exact in f32: what is left is the bf16 rounding of the
    result, the bound tests/test_fp8_gpu.py holds the e4m3 kernel to."""
    from kvq import nnops
    x, w, bias, x8, sx, w8, sw, prod = _operands(*shape)
    out = nnops.gemm_fp8_nt(x8, w8, sx, sw, bias=bias if with_bias else None, a_format="e5m2")
    ref = prod + (bias.float() if with_bias else 0.0)
    err = (out.float() - ref).abs().max().item()
    print(shape, with_bias, "max err", err, "bound", 2.0 ** -8 * ref.abs().max().item() + 1e-3)
    assert err <= 2.0 ** -8 * ref.abs().max().item() + 1e-3, err
    # ... and the two quantisations stay within the formats' resolution of the bf16 product: independent roundings to m mantissa bits
    # have an rms relative error of about 0.72 * 2^-(m+1) / sqrt(3) -- 0.052 for e5m2, 0.026 for e4m3, 0.058 together; twice that
    true = x.float() @ w.float().t() + (bias.float() if with_bias else 0.0)
    rel = (out.float() - true).norm().item() / true.norm().item()
    assert rel < 0.12, rel


def test_extended_entry_with_e4m3_and_no_accumulate_is_the_old_entry_bit_for_bit():
    from kvq import nnops
    for M, N, K in [(512, 768, 256), (1000, 776, 384)]:
        g = torch.Generator(device="cuda").manual_seed(M)
        x = torch.randn((M, K), generator=g, device="cuda").to(torch.bfloat16)
        w = (torch.randn((N, K), generator=g, device="cuda") * 0.05).to(torch.bfloat16)
        bias = torch.randn(N, generator=g, device="cuda").to(torch.bfloat16)
        x8, sx = nnops.fp8_quantize(x)
        w8, sw = nnops.fp8_quantize(w)
        old = nnops.gemm_fp8_nt(x8, w8, sx, sw, bias=bias)
        new = nnops.gemm_fp8_nt(x8, w8, sx, sw, bias=bias, a_format="e4m3")
        assert torch.equal(old.view(torch.int16), new.view(torch.int16))


def test_mixed_format_gemm_accumulates_into_its_output():
    """accumulate: C_old + product to the bound of the plain product, 2^-8 max|ref| + 1e-3.  The kernel rounds twice (the product to
    bf16, then the sum): its error is at most 2^-9 max|product| + half an ulp of the sum.  The operands are chosen so that the bound
    covers that whatever the bits: |C_old| <= 3 and |product| < 1 put max|ref| into [2.5, 4), where half an ulp is 2^-7, and
    2^-9 + 2^-7 <= 2^-8 * 2.5 + 1e-3.  (A missing or doubled product would be off by ~0.5.)"""
    from kvq import nnops
    M, N, K = 512, 768, 256
    x, w, bias, x8, sx, w8, sw, prod = _operands(M, N, K, w_scale=0.01, x_scale=1.0)
    g = torch.Generator(device="cuda").manual_seed(99)
    c_old = ((torch.rand((M, N), generator=g, device="cuda") * 6.0 - 3.0)).to(torch.bfloat16)
    ref = c_old.float() + prod
    assert prod.abs().max().item() < 1.0 and 2.5 <= ref.abs().max().item() < 4.0 and c_old.float().abs().max().item() <= 3.0
    out = nnops.gemm_fp8_nt(x8, w8, sx, sw, out=c_old.clone(), a_format="e5m2", accumulate=True)
    err = (out.float() - ref).abs().max().item()
    print("accumulate: max err", err, "bound", 2.0 ** -8 * ref.abs().max().item() + 1e-3)
    assert err <= 2.0 ** -8 * ref.abs().max().item() + 1e-3, err


# ---- 4 - 6. the engine ---------------------------------------------------------------------------------------------------------------
def _build(seed=0):
    """(the _build of tests/test_fp8_gpu.py: bert-base widths, 2 + 2 layers, 512 codes)"""
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(seed)
    vq = VectorQuantizer(512, 768, 0.25, vq_codebook_init_values=torch.randn(512, 768))
    vq.materialize_min_encodings = False
    return Shelgon("kvq-bert-base-2l", vq, "kvq-bert-base-2l", None, compute_dtype=torch.bfloat16).cuda().eval()


def _batch(seed):
    from dsentences.synthetic import random_token_batch
    return tuple(t.cuda() for t in random_token_batch(8, 32, torch.Generator().manual_seed(seed)))      # 256 rows: the smallest eligible batch


def _expected_sites(eng, rows):
    """The fp8 input-gradient launches of one step, from the model's shapes: every product gx = gy . W of the backward schedule whose
    weight has an fp8 segment and whose contraction length (the rows of W) is a multiple of 128.  Per layer: attention output,
    fused q|k|v, [decoder: cross-attention output and query,] BertIntermediate -- and BertOutput only where the schedule does not
    fold its input gradient into the GELU' GEMM (a tile decision from the shapes); the all-layer cross-K/V block; the head's
    transform.  The LM head contracts over the padded vocabulary (30528 = 238.5 x 128): bf16."""
    H, I = eng.H, eng.ecfg.intermediate_size
    assert rows >= 256 and H % 128 == 0 and I % 128 == 0 and (2 * H * eng.n_dec_layers) % 128 == 0 and eng.Vp % 128 != 0
    f2_fused = eng._epilogue_tile(rows, I, H) is not None
    want = []
    for side, n, names in (("enc", eng.n_enc_layers, ("sa.o.w", "sa.q.w", "f1.w")),
                           ("dec", eng.n_dec_layers, ("sa.o.w", "sa.q.w", "ca.o.w", "ca.q.w", "f1.w"))):
        for i in range(n):
            want += [f"{side}.{i}.{nm}" for nm in names] + ([] if f2_fused else [f"{side}.{i}.f2.w"])
    assert eng._cakv_batched
    return sorted(want + [eng._cakv_w[0], "head.t.w"])


@pytest.fixture(scope="module")
def pair():
    """Two engines on the same weights, fp8 forward, lr = 0 (identical weights and forward bits on every step), with and without
    fp8_backward: three training steps each, what every step left behind."""
    from kvq.engine import TrainEngine
    ids, mask = _batch(4)
    runs = {}
    for bwd in (False, True):
        eng = TrainEngine(_build(), lr=0.0, fp8_forward=True, fp8_backward=bwd)
        steps = []
        for _ in range(3):
            out = eng.train_step(ids, mask)
            torch.cuda.synchronize()
            grads = {n: eng.flat.g(n).clone() for n, p in eng.param_of.items() if p.requires_grad}
            grads["codebook"] = eng.gE.clone()
            steps.append(dict(loss=(out["loss_recon"].clone(), out["loss_vq"].clone()), grads=grads, launches=eng.fp8_bwd_launches,
                              sites=list(eng.fp8_bwd_sites)))
        runs[bwd] = (eng, steps)
    return runs


def test_first_step_calibrates_on_bf16_and_the_second_runs_every_eligible_site_on_fp8(pair):
    (e0, s0), (e1, s1) = pair[False], pair[True]
    assert not e0.fp8_backward and e0.fp8_bwd_launches == 0 and e0._w8t is None
    # step 1: every input gradient on bf16 (the sites only note their amax) -- the gradients of the engine without the option, bitwise
    assert s1[0]["launches"] == 0 and s1[0]["sites"] == []
    for n, g in s0[0]["grads"].items():
        assert torch.equal(g, s1[0]["grads"][n]), n
    for a, b in zip(s0[0]["loss"], s1[0]["loss"]):
        assert torch.equal(a, b)
    # ... and every site the step visited left with a scale from its measured amax (57344 / (4 amax)); a site it did not visit
    # keeps scale 0 and stays on bf16
    want = _expected_sites(e1, 256)
    sc = e1._g8_state[:, 0].cpu()
    assert e1._g8_ready and sorted(e1._g8_live) == want
    for key, i in e1._g8_index.items():
        assert (sc[i].item() > 0 and np.isfinite(sc[i].item())) if key in want else sc[i].item() == 0.0, key
    # step 2
    assert s1[1]["launches"] == len(want) > 0 and sorted(s1[1]["sites"]) == want
    assert "dec.emb.word" not in e1._g8_index and "dec.emb.word" in e1._w8_index       # the LM head stays bf16
    # the transposed mirror is the transpose of the mirror
    for key in want:
        d, M, K = e1._w8t_seg[key]
        o = e1.flat.seg[key][0]
        assert torch.equal(e1._w8t[d:d + M * K].view(K, M), e1._w8[o:o + M * K].view(M, K).t()), key


def test_gradients_against_the_bf16_backward_on_identical_forward_bits(pair):
    """Step 3 (replayed from the captured graphs in both engines), lr = 0: the losses are equal bitwise -- the forward does not know
    about the option -- and the gradients point the way of the bf16 backward: cosine > 0.9 per tensor, > 0.98 on average, the
    thresholds tests/test_fp8_gpu.py holds the fp8 forward to (as there without the key biases, whose true gradient is zero: a
    constant added to every score of a softmax row).  Measured on MI355X: profiles/fp8_dgrad.md."""
    (e0, s0), (e1, s1) = pair[False], pair[True]
    assert e0._graphs and e1._graphs and s1[2]["launches"] == s1[1]["launches"] and s1[2]["sites"] == s1[1]["sites"]      # (a replay restores its graphs' counts)
    for a, b in zip(s0[2]["loss"], s1[2]["loss"]):
        assert torch.equal(a, b)
    g0, g1 = s0[2]["grads"], s1[2]["grads"]
    cos = {n: F.cosine_similarity(g1[n].float().reshape(-1), g0[n].float().reshape(-1), dim=0).item()
           for n in g0 if g0[n].float().norm() > 0 and not n.endswith("k.b")}
    worst = min(cos, key=cos.get)
    print(f"fp8 input gradients against bf16: {len(cos)} tensors, min cosine {cos[worst]:.5f} ({worst}), mean {np.mean(list(cos.values())):.5f}")
    assert all(torch.isfinite(g1[n].float()).all() for n in g1)
    assert cos[worst] > 0.9 and np.mean(list(cos.values())) > 0.98, (worst, cos[worst], np.mean(list(cos.values())))
    assert any(not torch.equal(g0[n], g1[n]) for n in g0)                              # (the option did change the backward)


def test_replayed_steps_equal_eager_steps():
    """Four training steps with fp8_backward (dropout on, lr > 0): step 1 calibrates, 2 is eager, 3 is captured, 4 replayed -- against
    four eager steps of an engine on the same weights.  Master weights and codebook bit-identical; the captured graphs hold
    kernel nodes only (the e5m2 passes, the segmented transpose and the scale update are kernels)."""
    from kvq.engine import TrainEngine
    ids, mask = _batch(5)
    res = {}
    for graph in (False, True):
        eng = TrainEngine(_build(1).train(), lr=2e-4, fp8_forward=True, fp8_backward=True)
        eng.use_graph = graph
        losses = [float(eng.train_step(ids, mask)["loss_recon"]) for _ in range(4)]
        torch.cuda.synchronize()
        assert np.isfinite(losses).all() and eng.fp8_bwd_launches > 0
        res[graph] = (eng, eng.flat.master.clone(), eng.E.data.clone(), losses)
    (_, w0, c0, l0), (eg, w1, c1, l1) = res[False], res[True]
    assert eg._graphs and not res[False][0]._graphs
    assert l0 == l1, (l0, l1)
    assert torch.equal(w0, w1) and torch.equal(c0, c1)
    census = next(iter(eg._graphs.values())).node_census()
    print("graphs of the step chain:", census)
    for c in census:
        assert c["memset"] == 0 and c["memcpy"] == 0 and c["other"] == 0, census


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from kvq import nnops
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    with pytest.raises(KvqError, match="fp8_backward needs fp8 forward"):
        TrainEngine(_build(), fp8_forward=False, fp8_backward=True)
    a8 = torch.zeros((256, 192), dtype=torch.uint8, device="cuda")
    b8 = torch.zeros((64, 192), dtype=torch.uint8, device="cuda")
    one = torch.ones(1, device="cuda")
    with pytest.raises(KvqError, match="K % 128"):
        nnops.gemm_fp8_nt(a8, b8, one, one, a_format="e5m2")
    with pytest.raises(KvqError, match="format"):
        nnops.gemm_fp8_nt(a8[:, :128], b8[:, :128], one, one, a_format=2)
    with pytest.raises(KvqError, match="multiples of 16"):
        nnops.fp8_transpose(torch.zeros((24, 32), dtype=torch.uint8, device="cuda"))
    with pytest.raises(KvqError, match="format"):
        nnops.fp8_quantize(torch.zeros((16, 16), dtype=torch.bfloat16, device="cuda"), fmt="e3m4")
