"""TrainEngine(max_grad_norm=...): the global gradient norm measured inside the step, clipping by it and the skip of a non-finite
step -- against the per-parameter gradients (the padding of the flat buffer must stay out of the norm), torch.optim.Adam fed the
clipped gradients, the eager step against the hipGraph replay, and an engine built without the option."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, S = 16, 12


def _shelgon(dtype, name="kvq-bert-tiny-nodrop"):
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(0)
    vq = VectorQuantizer(32, 128, 0.25, vq_codebook_init_values=torch.randn(32, 128))
    vq.materialize_min_encodings = False
    model = Shelgon(name, vq, name, None, compute_dtype=dtype).cuda()
    model.set_mode("full")
    return model.train()


def _bagon(dtype, name="kvq-bert-tiny-nodrop"):
    from models.bagon.Bagon import Bagon
    torch.manual_seed(0)
    model = Bagon(name, name, True, compute_dtype=dtype).cuda()
    model.set_mode("full")
    return model.train()


def _batch(seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(3, S + 1, (B,), generator=g)
    ids = ids * (torch.arange(S)[None] < lens[:, None])
    noise = torch.randint(1000, 2000, (B, S), generator=g)
    dec = torch.where(torch.rand((B, S), generator=g) < 0.3, noise, ids) * (ids != 0)
    mask = (ids != 0).long()
    return ids.cuda(), mask.cuda(), dec.cuda()


def _step_kw(eng, dec, mask):
    return {} if eng.has_vq else dict(dec_ids=dec, dec_mask=mask)          # Bagon: decoder ids that differ from the encoder's


def _norm64(eng):
    return math.sqrt(sum((g.double() ** 2).sum().item() for g in eng.grads_by_parameter().values()))


@pytest.fixture(autouse=True)
def _no_environment_switch(monkeypatch):
    monkeypatch.delenv("KVQ_MAX_GRAD_NORM", raising=False)


@pytest.mark.parametrize("kind", ["shelgon", "bagon"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_grad_norm_is_the_norm_over_the_parameter_gradients(kind, dtype):
    """The padding test: the flat gradient buffer also holds alignment padding and the padded rows of the vocabulary table; the
    norm is over what torch.nn.utils.clip_grad_norm_(model.parameters()) would see."""
    from kvq.engine import TrainEngine
    model = (_shelgon if kind == "shelgon" else _bagon)(dtype)
    eng = TrainEngine(model, lr=1e-3, max_grad_norm=float("inf"))
    eng.use_graph = False
    ids, mask, dec = _batch()
    out = eng.train_step(ids, mask, **_step_kw(eng, dec, mask))
    want = _norm64(eng)                                       # the step's gradients are still in the buffers (coef = 1 scales nothing)
    got = out["grad_norm"].item()
    print(f"{kind} {dtype}: grad_norm {got!r}, f64 norm over grads_by_parameter() {want!r}, rel {abs(got - want) / want:.3g}; "
          f"pieces {len(eng.flat.pieces)}, ranges {len(eng.flat.ranges)}")
    assert out["grad_norm"].dtype == torch.float32 and out["grad_norm"].is_cuda and out["grad_clip_coef"].item() == 1.0
    assert want > 0 and abs(got - want) <= 1e-6 * want
    assert eng.skipped_steps == 0


@pytest.mark.parametrize("mode", ["dec-head-ft", "enc-head-ft-dec-head-ft"])
def test_grad_norm_in_the_freeze_modes(mode):
    """Partial-training modes: several trainable ranges with frozen entries between them -- several pieces, the same norm."""
    from kvq.engine import TrainEngine
    model = _shelgon(torch.float32)
    model.set_mode(mode)
    eng = TrainEngine(model.train(), lr=1e-3, max_grad_norm=float("inf"))
    eng.use_graph = False
    ids, mask, _ = _batch()
    out = eng.train_step(ids, mask)
    want, got = _norm64(eng), out["grad_norm"].item()
    print(f"{mode}: grad_norm {got!r}, f64 {want!r}, pieces {len(eng.flat.pieces)}")
    assert len(eng.flat.pieces) > 1 and want > 0 and abs(got - want) <= 1e-6 * want


def test_a_bound_never_reached_changes_no_bit():
    """max_grad_norm = 1e9: coef is 1.0f and x * 1.0f is exact -- weights, moments and codebook of four steps (two eager, then
    captured and replayed) are those of an engine built without the option from the same seed."""
    from kvq.engine import TrainEngine
    ids, mask, _ = _batch()
    runs = []
    for mgn in (None, 1e9):
        eng = TrainEngine(_shelgon(torch.bfloat16), lr=1e-3, max_grad_norm=mgn)
        for _ in range(4):
            out = eng.train_step(ids, mask)
        torch.cuda.synchronize()
        assert eng._graphs
        assert ("grad_norm" in out) == (mgn is not None)
        runs.append((eng.flat.master.clone(), eng.flat.m.clone(), eng.flat.v.clone(), eng.flat.shadow.clone(), eng.E.detach().clone(),
                     eng.aux[0]["m"].clone(), eng.aux[0]["v"].clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert float(out["grad_clip_coef"]) == 1.0 and math.isfinite(float(out["grad_norm"]))


def test_clipped_steps_match_torch_adam_on_the_clipped_gradients():
    from kvq.engine import TrainEngine
    ids, mask, _ = _batch(seed=3)
    probe = TrainEngine(_shelgon(torch.float32), lr=1e-3, max_grad_norm=float("inf"))
    probe.use_graph = False
    max_norm = 0.5 * probe.train_step(ids, mask)["grad_norm"].item()
    model = _shelgon(torch.float32)
    eng = TrainEngine(model, lr=1e-3, max_grad_norm=max_norm)
    eng.use_graph = False
    params = [p for p in eng.param_of.values() if p.requires_grad] + [a["p"] for a in eng.aux if a["p"].requires_grad]
    clones = {p: p.detach().clone().requires_grad_(True) for p in params}
    opt = torch.optim.Adam(list(clones.values()), lr=1e-3)
    for step in range(3):
        out = eng.train_step(ids, mask)
        grads = eng.grads_by_parameter()
        assert set(grads) == set(params)
        coef = min(1.0, max_norm / (_norm64(eng) + 1e-6))                       # clip_grad_norm_'s formula in f64
        got_coef = out["grad_clip_coef"].item()
        print(f"step {step + 1}: grad_norm {out['grad_norm'].item():.6g}, grad_clip_coef {got_coef!r}, f64 {coef!r}")
        assert got_coef < 1.0 and abs(got_coef - coef) <= 1e-6 * coef
        for p, c in clones.items():
            c.grad = (grads[p].double() * coef).float()
        opt.step()
        for p, c in clones.items():
            torch.testing.assert_close(p.data, c.data, rtol=2e-6, atol=2e-7)


def test_replayed_steps_equal_eager_steps_bit_for_bit(monkeypatch):
    monkeypatch.setenv("KVQ_GRAPH_STRICT", "1")
    from kvq.engine import TrainEngine
    ids, mask, _ = _batch(seed=4)
    runs = []
    for use_graph in (False, True):
        eng = TrainEngine(_shelgon(torch.bfloat16), lr=1e-3, max_grad_norm=0.25)
        eng.use_graph = use_graph
        norms, coefs = [], []
        for _ in range(6):
            out = eng.train_step(ids, mask)
            norms.append(out["grad_norm"])
            coefs.append(out["grad_clip_coef"])
        torch.cuda.synchronize()
        assert bool(eng._graphs) == use_graph and eng.step_count == 6
        if use_graph:
            census = next(iter(eng._graphs.values())).node_census()
            print("graphs of the step chain with max_grad_norm:", census)
            for c in census:
                assert c["memset"] == 0 and c["memcpy"] == 0 and c["other"] == 0, census
        runs.append((eng.flat.master.clone(), eng.E.detach().clone(), torch.stack(norms), torch.stack(coefs)))
    (p0, e0, n0, c0), (p1, e1, n1, c1) = runs
    print("grad_norm per step:", n0.tolist(), "replayed:", n1.tolist())
    assert len(set(n0.tolist())) == 6                         # every step handed out its own norm, not a view of the last one
    assert torch.equal(n0, n1) and torch.equal(c0, c1)
    assert torch.equal(p0, p1) and torch.equal(e0, e1)
    assert bool((c0 < 1).any())


def test_a_non_finite_gradient_skips_the_step_and_the_next_one_trains():
    from kvq import nnops
    from kvq.engine import TrainEngine
    ids, mask, _ = _batch(seed=5)
    eng = TrainEngine(_shelgon(torch.bfloat16), lr=1e-3, max_grad_norm=1.0)
    eng.use_graph = False
    eng.train_step(ids, mask)                                 # one ordinary step: the moments are not zero any more
    eng.forward_backward(ids, mask, compute_grads=True)
    eng.flat.grad[eng.flat.seg["enc.0.f1.w"][0] + 77] = float("inf")
    fl = eng.flat
    before = [t.clone() for t in (fl.master, fl.m, fl.v, fl.shadow, eng.E.data, eng.aux[0]["m"], eng.aux[0]["v"])]
    step0 = eng.step_count
    eng.optimizer_step()
    torch.cuda.synchronize()
    after = (fl.master, fl.m, fl.v, fl.shadow, eng.E.data, eng.aux[0]["m"], eng.aux[0]["v"])
    for a, b in zip(before, after):
        assert torch.equal(a.view(torch.int16) if a.element_size() == 2 else a.view(torch.int32),
                           b.view(torch.int16) if b.element_size() == 2 else b.view(torch.int32))
    st = nnops.read_grad_guard(eng._guard)
    assert eng.skipped_steps == 1 and st["skip"] == 1 and st["coef"] == 0.0
    assert eng.step_count == step0 + 1 and nnops.read_step_state(eng._state)[0] == step0 + 1       # the step state moved on
    out = eng.train_step(ids, mask)
    torch.cuda.synchronize()
    assert math.isfinite(out["grad_norm"].item()) and 0.0 < out["grad_clip_coef"].item() <= 1.0
    assert not torch.equal(before[0], fl.master) and not torch.equal(before[4], eng.E.data)
    assert eng.skipped_steps == 1 and nnops.read_grad_guard(eng._guard)["skip"] == 0


def test_off_by_default_and_bad_values_are_refused():
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    ids, mask, _ = _batch()
    model = _shelgon(torch.bfloat16)
    eng = TrainEngine(model, lr=1e-3)
    eng.use_graph = False
    out = eng.train_step(ids, mask)
    assert "grad_norm" not in out and "grad_clip_coef" not in out
    assert eng.max_grad_norm is None and eng._guard is None and eng.skipped_steps == 0
    for bad in (-1, 0, float("nan"), "1.0", True):
        with pytest.raises(KvqError, match="max_grad_norm"):
            TrainEngine(model, max_grad_norm=bad)
