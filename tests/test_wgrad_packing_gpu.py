"""The packed weight-gradient schedule (kvq/engine.py above _flush_wgrads): (1) the mixed-tile grouped launch
stores, for every problem, the bits the single-shape grouped launch stores on the same tile, and nothing else; (2) the engine's
gradients with the packed schedule are the bits of the unpacked one (KVQ_WG_PACK=0), and the launches are the ones the tile counts
give; (3) the packed step captured and replayed is the eager step, bit for bit.  "bits equal" = equality of the raw words."""
import pytest
import torch

pytestmark = pytest.mark.gpu

T256, T128 = "256x256", "128x256"


@pytest.fixture(autouse=True)
def _no_environment_switch(monkeypatch):
    for name in ("KVQ_WG_PACK", "KVQ_DP_SINGLE_RANK", "KVQ_GRAPH", "KVQ_OWN_GEMM", "KVQ_GEMM_TILE", "KVQ_GEMM_BAND", "KVQ_GRAD_ACCUM"):
        monkeypatch.delenv(name, raising=False)


def _raw(t):
    return t.detach().contiguous().reshape(-1).view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------------------
GUARD = 8        # guard rows above and below, guard columns (8 = 16 bytes: the output stays 16-byte aligned) left and right


class _Problem:
    """One TN problem C[M, N] = A[K, M]^T . B[K, N] on random bf16 operands; A may be a column slice of a wider tensor.  Every
    output is a window of a NaN-filled buffer with GUARD rows / columns around it."""

    def __init__(self, M, N, K, seed, a_cols=None, a_off=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        wide = torch.randn((K, a_cols or M), generator=g, device="cuda").to(torch.bfloat16)
        self.a = wide[:, a_off:a_off + M]
        self.b = torch.randn((K, N), generator=g, device="cuda").to(torch.bfloat16)
        self.M, self.N = M, N

    def out(self):
        buf = torch.full((self.M + 2 * GUARD, self.N + 2 * GUARD), float("nan"), dtype=torch.bfloat16, device="cuda")
        return buf, buf[GUARD:GUARD + self.M, GUARD:GUARD + self.N]

    def problem(self, window):
        from kvq import nnops
        return nnops.gemm_problem(self.a, self.b, window, "tn")


def _inside(buf):
    m = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    m[GUARD:-GUARD, GUARD:-GUARD] = True
    return m


@pytest.fixture(scope="module")
def mixed_cases():
    """The three problems of the issue and, once, what the single-shape grouped launch stores for each alone on its tile."""
    from kvq import nnops
    cases = [(_Problem(392, 264, 256, 1), T256),                         # one whole 256 x 256 tile, ragged edges in both directions
             (_Problem(136, 768, 256, 2), T128),                         # three tile columns, a ragged second tile row
             (_Problem(128, 256, 256, 3, a_cols=512, a_off=256), T128)]  # a column slice of a [K, 512] tensor: lda = 512 != M
    assert cases[2][0].a.stride(0) == 512
    refs = []
    for p, tile in cases:
        buf, win = p.out()
        nnops.gemm_grouped([p.problem(win)], "tn", tile)
        torch.cuda.synchronize()
        assert torch.isfinite(win.float()).all()
        refs.append(buf)
    return cases, refs


@pytest.mark.parametrize("which", [(0, 1, 2), (2, 0, 1), (0,), (1, 2)], ids=["mixed", "mixed-small-first", "only-256", "only-128"])
def test_mixed_launch_stores_the_bits_of_the_single_shape_launch_and_nothing_else(mixed_cases, which):
    from kvq import nnops
    cases, refs = mixed_cases
    bufs, probs, tiles = [], [], []
    for i in which:
        p, tile = cases[i]
        buf, win = p.out()
        bufs.append(buf)
        probs.append(p.problem(win))
        tiles.append(tile)
    nnops.gemm_grouped_mixed(probs, tiles, "tn")
    torch.cuda.synchronize()
    for i, buf in zip(which, bufs):
        inside = _inside(buf)
        assert torch.equal(_raw(buf[GUARD:-GUARD, GUARD:-GUARD]), _raw(refs[i][GUARD:-GUARD, GUARD:-GUARD])), f"problem {i}: bits differ"
        assert torch.isnan(buf[~inside]).all(), f"problem {i}: written outside its output"
        assert torch.equal(_raw(buf), _raw(refs[i])), f"problem {i}: guard bits differ"


def test_mixed_launch_refuses_17_problems_and_other_tiles(mixed_cases):
    from kvq import nnops
    from kvq._ffi import KvqError
    cases, _ = mixed_cases
    p, _ = cases[2]
    buf, win = p.out()
    with pytest.raises(KvqError):
        nnops.gemm_grouped_mixed([p.problem(win)] * 17, [T128] * 17, "tn")
    with pytest.raises(KvqError):
        nnops.gemm_grouped_mixed([p.problem(win)], ["128x192"], "tn")
    with pytest.raises(KvqError):
        nnops.gemm_grouped_mixed([p.problem(win)], [T128, T128], "tn")
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()                    # a refused launch wrote nothing


# ---- 2. / 3. the engine ----------------------------------------------------------------------------------------------------------------
def _build_base():
    """kvq-bert-base-2l Shelgon in bf16 (the setup of the data-parallel tests at bert-base widths)."""
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(0)
    vq = VectorQuantizer(512, 768, 0.25, vq_codebook_init_values=torch.randn(512, 768))
    vq.materialize_min_encodings = False
    model = Shelgon("kvq-bert-base-2l", vq, "kvq-bert-base-2l", None, compute_dtype=torch.bfloat16).cuda()
    model.set_mode("full")
    return model.eval()


def _data_base():
    from dsentences.synthetic import random_token_batch
    ids, mask = random_token_batch(64, 32, torch.Generator().manual_seed(11))        # 64 x 32 = 2048 tokens
    return ids.cuda(), mask.cuda()


def _poison(eng):
    eng.flat.grad.fill_(float("nan"))
    for a in eng.aux:
        a["g"].fill_(float("nan"))


def _grad_snapshot(eng):
    torch.cuda.synchronize()
    out = {n: eng.flat.g(n).detach().clone() for n, p in eng.param_of.items() if p.requires_grad}
    out["codebook"] = eng.gE.detach().clone()
    return out


def _record_tn_launches(monkeypatch, log):
    """Wrap the three ways a weight gradient reaches the library; log gets (kind, [(tile, (M, N)), ...]) per launch."""
    from kvq import nnops
    grouped, mixed, single = nnops.gemm_grouped, nnops.gemm_grouped_mixed, nnops.gemm

    def w_grouped(problems, layout, tile):
        if layout == "tn":
            log.append(("grouped", sorted((tile, (p.M, p.N)) for p in problems)))
        return grouped(problems, layout, tile)

    def w_mixed(problems, tiles, layout="tn"):
        log.append(("mixed", sorted((t, (p.M, p.N)) for p, t in zip(problems, tiles))))
        return mixed(problems, tiles, layout)

    def w_single(a, b, layout="nt", **kw):
        if layout == "tn":
            log.append(("single", [(kw.get("tile"), (a.shape[1], b.shape[1]))]))
        return single(a, b, layout, **kw)
    monkeypatch.setattr(nnops, "gemm_grouped", w_grouped)
    monkeypatch.setattr(nnops, "gemm_grouped_mixed", w_mixed)
    monkeypatch.setattr(nnops, "gemm", w_single)


def _tiles(launch):
    return sum(-(-M // (256 if t == T256 else 128)) * -(-N // 256) for t, (M, N) in launch[1])


# kvq-bert-base-2l, H = 768, FFN 3072, vocabulary padded to 30528: weight-gradient shapes [out, in] and their 256 x 256 tile counts
H, F, VP = 768, 3072, 30528
ENC_LAYER = [(3 * H, H), (H, H), (F, H), (H, F)]                         # fused Q/K/V 27, attention output 9, FFN 36 + 36 = 108
DEC_LAYER = ENC_LAYER + [(H, H), (H, H)]                                 # + cross-attention query and output 9 + 9 = 126
CAKV_SLICE = (2 * H, H)                                                  # one layer's cross-attention key / value rows: 18


def _g(tile, shapes):
    return sorted((tile, s) for s in shapes)


# 256 CUs, three 256-wide tile columns.
#   LM head: 85 tile rows = 21760 vocabulary rows = 255 tiles of 256 x 256 fill the CUs once; the other 8768 rows are 69 x 3 = 207
#   tiles of 128 x 256, the launch's second, shorter round: ONE launch through nnops.gemm(tile="mixed") -> the mixed-tile call.
#   head.t.w (9 tiles) and the batched cross-K/V gradient ([3072, 768]: 2 per-layer slices of 18) wait for idle CUs:
#   the decoder pair (252) has 4 idle CUs = one 256-row slice of head.t.w (3 tiles): 255;
#   the encoder pair (216) has 40: both cross-K/V slices (36, contiguous rows: one problem) and one more slice of head.t.w: 255.
#   252 + 216 + 9 + 36 = 513 tiles do not fit two rounds of 256: the last 256 rows of head.t.w (6 tiles of 128 x 256) go out with
#   the forced flush that ends backward.  (The 12-layer model has 12 such rounds for 9 + 216 waiting tiles: nothing is left over.)
PACKED = [("single", [("mixed", (VP, H))]),
          ("mixed", sorted(_g(T256, [(21760, H)]) + _g(T128, [(VP - 21760, H)]))),
          ("grouped", _g(T256, 2 * DEC_LAYER + [(256, H)])),
          ("grouped", _g(T256, 2 * ENC_LAYER + [(4 * H, H), (256, H)])),
          ("grouped", _g(T128, [(256, H)]))]
# The unpacked schedule: LM head alone (tile by the cost model); head.t.w (9) + decoder 1 (126) = 135 tiles, which no second layer
# fits beside; decoder 0 (126) + the batched cross-K/V gradient ([3072, 768]: 36) = 162; the encoder pair, 216.
UNPACKED = [("single", [(None, (VP, H))]),
            ("grouped", _g(T256, [(H, H)] + DEC_LAYER)),
            ("grouped", _g(T256, DEC_LAYER + [(4 * H, H)])),
            ("grouped", _g(T256, 2 * ENC_LAYER))]


def _two_steps(pack, monkeypatch):
    from kvq.engine import TrainEngine
    monkeypatch.setenv("KVQ_WG_PACK", "1" if pack else "0")
    eng = TrainEngine(_build_base(), lr=0.0)
    eng.use_graph = False
    assert eng._wg_pack == pack and not eng._dp and eng._own_wgrad and eng._cakv_batched and eng._n_cu == 256
    ids, mask = _data_base()
    log, grads = [], None
    for step in range(2):
        _poison(eng)
        with monkeypatch.context() as m:
            if step == 1:
                _record_tn_launches(m, log)
            eng.train_step(ids, mask)
        grads = _grad_snapshot(eng)
    return grads, log


def test_engine_gradients_are_the_unpacked_bits_and_the_launches_are_the_packed_ones(monkeypatch):
    """kvq-bert-base-2l, bf16, 64 x 32 tokens, one process, lr = 0, gradient buffers NaN-filled before each step: every trainable
    gradient and the codebook gradient are finite and bit-identical with the packed schedule and with KVQ_WG_PACK=0, and the TN
    launches of one backward are the lists above.  (The LM head stays ONE launch of nnops.gemm -- on the mixed tile -- and head.t.w
    waits for idle CUs like the cross-K/V slices instead of joining the LM-head launch: the tests that judge every GEMM of a step
    against f32 need that single weight-gradient launch.  At 2 + 2 layers one 256-row slice of head.t.w is left for the forced flush.)"""
    packed, log_p = _two_steps(True, monkeypatch)
    torch.cuda.empty_cache()
    plain, log_u = _two_steps(False, monkeypatch)
    assert set(packed) == set(plain) and "codebook" in packed and "dec.emb.word" in packed
    for n in packed:
        assert torch.isfinite(packed[n].float()).all() and torch.isfinite(plain[n].float()).all(), n
    bad = [n for n in packed if not torch.equal(_raw(packed[n]), _raw(plain[n]))]
    assert not bad, f"gradient bits differ between the packed and the unpacked schedule: {bad}"
    count = lambda log: [(k, _tiles((k, l)) if k != "single" else None) for k, l in log]  # noqa: E731
    print("packed launches:", count(log_p), "unpacked:", count(log_u))
    assert log_p == PACKED, log_p
    assert log_u == UNPACKED, log_u
    # what the packing is for: no launch of cross-K/V rows alone, no 128 x 256 launch of a transformer layer, the layers' rounds
    # full and within the CUs
    cakv = {(4 * H, H), (2 * H, H)}
    assert not any(k == "grouped" and {s for _, s in l} <= cakv for k, l in log_p)
    assert not any(k == "grouped" and t == T128 and s in ENC_LAYER for k, l in log_p for t, s in l)
    assert [_tiles(x) for x in log_p[1:]] == [255 + 207, 255, 255, 6]


def _snapshot(eng):
    torch.cuda.synchronize()
    fl = eng.flat
    out = {"master": fl.master, "shadow": fl.shadow, "m": fl.m, "v": fl.v, "state": eng._state, "codebook": eng.E.data}
    for i, a in enumerate(eng.aux):
        out.update({f"aux{i}.{k}": a[k] for k in ("m", "v")})
    return {k: v.detach().clone() for k, v in out.items()}


def test_captured_packed_step_is_the_eager_step_bit_for_bit():
    """Four steps with lr = 1e-4 and the packed schedule, captured and replayed against launched eagerly: master and shadow weights,
    Adam moments, step state, codebook and every tensor a step returns are bit-equal after each step; the graphs hold kernels only."""
    from kvq.engine import TrainEngine
    ids, mask = _data_base()
    engines = []
    for use_graph in (False, True):
        eng = TrainEngine(_build_base(), lr=1e-4)
        eng.use_graph = use_graph
        assert eng._wg_pack and not eng._dp
        engines.append(eng)
    eager, graph = engines
    for step in range(1, 5):                          # the third call captures, the fourth replays
        oe, og = eager.train_step(ids, mask), graph.train_step(ids, mask)
        keys = sorted(k for k in oe if torch.is_tensor(oe[k]))
        assert keys == sorted(k for k in og if torch.is_tensor(og[k])) and "loss_recon" in keys and "indices" in keys
        bad = [k for k in keys if not torch.equal(_raw(oe[k]), _raw(og[k]))]
        assert not bad, f"step {step}: outputs differ in {bad}"
        se, sg = _snapshot(eager), _snapshot(graph)
        bad = [k for k in se if not torch.equal(_raw(se[k]), _raw(sg[k]))]
        assert not bad, f"after step {step}: bits differ in {bad}"
        assert torch.isfinite(se["master"]).all()
    assert not eager._graphs and len(graph._graphs) == 1
    for census in next(iter(graph._graphs.values())).node_census():
        assert census["kernel"] > 0 and census["memset"] == census["memcpy"] == census["other"] == 0, census
