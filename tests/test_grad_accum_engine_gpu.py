"""TrainEngine(grad_accum=A): A micro-steps (forward, backward, the gradient added into an f32 accumulator) per optimiser step on the
mean of their gradients -- against the sequential torch sum of the micro-batch gradients, torch.optim.Adam fed the mean, one step on
the concatenated batch, the hipGraph replay against eager launches, and an engine built without the option."""
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


def _batch(seed=1, b=B):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (b, S), generator=g)
    lens = torch.randint(3, S + 1, (b,), generator=g)
    ids = ids * (torch.arange(S)[None] < lens[:, None])
    noise = torch.randint(1000, 2000, (b, S), generator=g)
    dec = torch.where(torch.rand((b, S), generator=g) < 0.3, noise, ids) * (ids != 0)
    mask = (ids != 0).long()
    return ids.cuda(), mask.cuda(), dec.cuda()


def _step_kw(eng, dec, mask):
    return {} if eng.has_vq else dict(dec_ids=dec, dec_mask=mask)          # Bagon: decoder ids that differ from the encoder's


def _norm64(eng):
    return math.sqrt(sum((g.double() ** 2).sum().item() for g in eng.grads_by_parameter().values()))


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _trainable_aux(eng):
    return [a for a in eng.aux if a["p"].requires_grad]


@pytest.fixture(autouse=True)
def _no_environment_switch(monkeypatch):
    for name in ("KVQ_GRAD_ACCUM", "KVQ_MAX_GRAD_NORM", "KVQ_VQ_REVIVE_AFTER", "KVQ_DP_SINGLE_RANK"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("kind", ["shelgon", "bagon"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_accumulator_is_the_sequential_f32_sum_of_the_micro_batch_gradients(kind, dtype):
    from kvq import nnops
    from kvq.engine import TrainEngine
    eng = TrainEngine((_shelgon if kind == "shelgon" else _bagon)(dtype), lr=1e-3, grad_accum=4)
    eng.use_graph = False
    assert eng.grad_accum == 4 and eng.accum_pending == 0
    w0 = eng.flat.master.clone()
    flat_g, aux_g = [], []
    for k in range(4):
        ids, mask, dec = _batch(seed=10 + k)
        out = eng.train_step(ids, mask, **_step_kw(eng, dec, mask))
        flat_g.append(eng.flat.grad.clone())
        aux_g.append([a["g"].clone() for a in _trainable_aux(eng)])
        assert out["optimizer_step"] is (k == 3) and eng.accum_pending == (k + 1) % 4
        assert torch.equal(eng.flat.master, w0) == (k < 3), k                 # the weights move on the fourth call only
    assert eng.step_count == 1 and nnops.read_accum_state(eng._acc_state) == (4, 0) and nnops.read_step_state(eng._state)[0] == 1
    quarter = torch.tensor(0.25, dtype=torch.float32, device="cuda")
    want = flat_g[0].float()
    for g in flat_g[1:]:
        want = want + g.float()
    want = want * quarter
    assert eng.flat.acc.dtype == torch.float32 and eng.flat.ranges
    for a, b in eng.flat.ranges:
        assert torch.equal(_bits(eng.flat.acc[a:b]), _bits(want[a:b])), (a, b)
    assert len(_trainable_aux(eng)) == (1 if kind == "shelgon" else 0)
    for i, a in enumerate(_trainable_aux(eng)):
        want = aux_g[0][i].float()
        for gs in aux_g[1:]:
            want = want + gs[i].float()
        assert torch.equal(_bits(a["acc"]), _bits(want * quarter))
    assert float(eng.flat.acc.abs().max()) > 0


def test_adam_consumes_the_mean():
    from kvq.engine import TrainEngine
    eng = TrainEngine(_shelgon(torch.float32), lr=1e-3, grad_accum=3)
    eng.use_graph = False
    params = [p for p in eng.param_of.values() if p.requires_grad] + [a["p"] for a in _trainable_aux(eng)]
    clones = {p: p.detach().clone().requires_grad_(True) for p in params}
    opt = torch.optim.Adam(list(clones.values()), lr=1e-3)
    for cycle in range(3):
        micro = []
        for k in range(3):
            ids, mask, _ = _batch(seed=20 + 3 * cycle + k)
            out = eng.train_step(ids, mask)
            if k < 2:
                micro.append(eng.grads_by_parameter())                         # a micro-step hands out its own gradient
        assert out["optimizer_step"] is True and eng.step_count == cycle + 1
        grads = eng.grads_by_parameter()                                        # the final one the mean Adam read
        assert set(grads) == set(params)
        probe = params[3]
        assert not torch.equal(grads[probe], micro[0][probe]) and not torch.equal(micro[0][probe], micro[1][probe])
        for p, c in clones.items():
            c.grad = grads[p].clone()
        opt.step()
        for p, c in clones.items():
            torch.testing.assert_close(p.data, c.data, rtol=2e-6, atol=2e-7)


def test_four_micro_batches_equal_one_step_on_their_concatenation():
    """Both loss terms are means over B * S rows, padding included: the mean of the gradients of four batches of 4 sentences is the
    gradient of the batch of 16.  f32, no dropout; the two differ in summation order only."""
    from kvq.engine import TrainEngine
    ids, mask, _ = _batch(seed=30)
    big = TrainEngine(_shelgon(torch.float32), lr=1e-3)
    out_big = big.forward_backward(ids, mask, compute_grads=True)
    want = big.grads_by_parameter()
    eng = TrainEngine(_shelgon(torch.float32), lr=1e-3, grad_accum=4)
    eng.use_graph = False
    codes = []
    for k in range(4):
        out = eng.train_step(ids[4 * k:4 * k + 4].contiguous(), mask[4 * k:4 * k + 4].contiguous())
        codes.append(out["indices"])
    assert out["optimizer_step"] is True
    assert torch.equal(torch.cat(codes), out_big["indices"])
    got = eng.grads_by_parameter()
    by_name = {big.param_of[n]: eng.param_of[n] for n in big.param_of}
    checked = 0
    for name, p in big.param_of.items():
        if p.requires_grad:
            torch.testing.assert_close(got[by_name[p]], want[p], rtol=2e-3, atol=2e-6, msg=lambda m: f"{name}: {m}")
            checked += 1
    assert checked > 10
    torch.testing.assert_close(got[eng.E], want[big.E], rtol=1e-4, atol=1e-8)


def test_replayed_micro_steps_equal_eager_ones_bit_for_bit(monkeypatch):
    """Dropout model: the masks come from the device's micro-step count in both runs."""
    monkeypatch.setenv("KVQ_GRAPH_STRICT", "1")
    from kvq import nnops
    from kvq.engine import TrainEngine
    batches = [_batch(seed=40 + k)[:2] for k in range(4)]
    runs = []
    for use_graph in (False, True):
        eng = TrainEngine(_shelgon(torch.bfloat16, "kvq-bert-tiny"), lr=1e-3, grad_accum=3)
        eng.use_graph = use_graph
        losses, ran = [], []
        for k in range(12):
            out = eng.train_step(*batches[k % 4])
            losses.append(out["loss_recon"])
            ran.append(out["optimizer_step"])
        torch.cuda.synchronize()
        assert ran == [False, False, True] * 4 and eng.step_count == 4 and eng.accum_pending == 0
        assert nnops.read_accum_state(eng._acc_state) == (12, 0) and nnops.read_step_state(eng._state)[0] == 4
        if use_graph:
            assert sorted(k[-1] for k in eng._graphs) == [False, True] and len({k[:3] for k in eng._graphs}) == 1      # both chains, one shape
            for key, chain in eng._graphs.items():
                census = chain.node_census()
                print("final" if key[-1] else "micro", "chain with grad_accum = 3:", census)
                for c in census:
                    assert c["kernel"] > 0 and c["memset"] == 0 and c["memcpy"] == 0 and c["other"] == 0, census
                    assert c["empty"] == 0 and c["event"] == 0, census            # kernel nodes only
        else:
            assert not eng._graphs
        fl, a = eng.flat, eng.aux[0]
        runs.append([t.clone() for t in (fl.master, fl.m, fl.v, fl.shadow, eng.E.data, fl.acc, a["acc"], a["m"], a["v"], torch.stack(losses))])
    for x, y in zip(*runs):
        assert torch.equal(_bits(x), _bits(y))


def test_fp8_gemms_need_nothing_special(monkeypatch):
    """fp8 forward and input-gradient GEMMs under accumulation (bert-base widths, 2 + 2 layers, 256 rows: the smallest eligible batch;
    dropout on): the activation scales move per micro-step, the weight mirrors are rewritten by the final step's Adam, which reads
    the f32 mean.  Eight calls at A = 2, both chains captured and replayed, against eager launches: bit-identical."""
    monkeypatch.setenv("KVQ_GRAPH_STRICT", "1")
    from dsentences.synthetic import random_token_batch
    from kvq.engine import TrainEngine
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    batches = [tuple(t.cuda() for t in random_token_batch(8, 32, torch.Generator().manual_seed(50 + k))) for k in range(2)]
    runs = []
    for use_graph in (False, True):
        torch.manual_seed(1)
        vq = VectorQuantizer(512, 768, 0.25, vq_codebook_init_values=torch.randn(512, 768))
        vq.materialize_min_encodings = False
        model = Shelgon("kvq-bert-base-2l", vq, "kvq-bert-base-2l", None, compute_dtype=torch.bfloat16).cuda().train()
        eng = TrainEngine(model, lr=2e-4, fp8_forward=True, fp8_backward=True, grad_accum=2)
        eng.use_graph = use_graph
        losses = [eng.train_step(*batches[k % 2])["loss_recon"] for k in range(8)]
        torch.cuda.synchronize()
        assert eng.step_count == 4 and eng.fp8_bwd_launches > 0 and bool(torch.isfinite(torch.stack(losses)).all())
        assert (sorted(k[-1] for k in eng._graphs) == [False, True]) if use_graph else not eng._graphs
        runs.append([t.clone() for t in (eng.flat.master, eng.flat.shadow, eng._w8, eng.E.data, eng.flat.acc, torch.stack(losses))])
    for x, y in zip(*runs):
        assert torch.equal(_bits(x), _bits(y))


def test_grad_accum_one_changes_no_bit():
    """grad_accum=1 against an engine built without the option: no buffer, the same graphs, the same bits (dropout model: the seeds
    still follow the step state)."""
    from kvq.engine import TrainEngine
    ids, mask, _ = _batch()
    runs, census = [], []
    for kw in ({}, dict(grad_accum=1)):
        eng = TrainEngine(_shelgon(torch.bfloat16, "kvq-bert-tiny"), lr=1e-3, **kw)
        for _ in range(4):
            out = eng.train_step(ids, mask)
        torch.cuda.synchronize()
        assert len(eng._graphs) == 1 and out["optimizer_step"] is True and eng.step_count == 4
        assert eng.grad_accum == 1 and eng._acc_state is None and eng.flat._acc is None and eng._seed_state is eng._state
        assert all("acc" not in a for a in eng.aux) and eng.accum_pending == 0
        census.append(next(iter(eng._graphs.values())).node_census())
        runs.append((eng.flat.master.clone(), eng.flat.m.clone(), eng.flat.v.clone(), eng.flat.shadow.clone(), eng.E.detach().clone(),
                     eng.aux[0]["m"].clone(), eng.aux[0]["v"].clone(), out["loss_recon"].clone()))
    assert census[0] == census[1]
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_dropout_masks_move_inside_a_cycle():
    """The optimiser step count stands still between the micro-steps of a cycle; the seeds follow the micro-step count, so the same
    batch twice gives two different gradients.  The learning-rate milestones count optimiser steps."""
    from kvq import nnops
    from kvq.engine import TrainEngine
    ids, mask, _ = _batch(seed=6)
    eng = TrainEngine(_shelgon(torch.float32, "kvq-bert-tiny"), lr=1e-3, grad_accum=2, milestones=[1], gamma=0.5)
    eng.use_graph = False
    eng.train_step(ids, mask)
    g0 = eng.flat.grad.clone()
    eng.train_step(ids, mask)
    g1 = eng.flat.grad.clone()
    assert not torch.equal(g0, g1) and float((g0 - g1).abs().max()) > 0
    assert nnops.read_accum_state(eng._acc_state) == (2, 0)
    step, lr = nnops.read_step_state(eng._state)[:2]
    assert step == 1 and lr == pytest.approx(1e-3, rel=1e-7)
    eng.train_step(ids, mask)
    eng.train_step(ids, mask)
    step, lr = nnops.read_step_state(eng._state)[:2]
    assert step == 2 and eng.step_count == 2 and lr == pytest.approx(1e-3 * 0.5, rel=1e-7)
    assert nnops.read_accum_state(eng._acc_state) == (4, 0)
    # the same engine without dropout would repeat itself: the difference above is the masks'
    nod = TrainEngine(_shelgon(torch.float32), lr=1e-3, grad_accum=2)
    nod.use_graph = False
    nod.train_step(ids, mask)
    h0 = nod.flat.grad.clone()
    nod.train_step(ids, mask)
    scale = float(h0.abs().max())
    moved, repeat = float((g0 - g1).abs().max()) / float(g0.abs().max()), float((h0 - nod.flat.grad).abs().max()) / scale
    print(f"largest gradient difference between two micro-steps on one batch, relative to the largest gradient: "
          f"with dropout {moved:.3g}, without {repeat:.3g}")
    assert repeat <= 1e-5 < 1e-2 <= moved          # new masks change the gradient by O(1); without them only the summation order could


def test_guard_runs_on_the_final_micro_step_and_a_poisoned_cycle_is_skipped():
    from kvq import nnops
    from kvq.engine import TrainEngine
    ids, mask, _ = _batch(seed=7)
    ids2, mask2, _ = _batch(seed=8)
    eng = TrainEngine(_shelgon(torch.bfloat16), lr=1e-3, grad_accum=2, max_grad_norm=float("inf"))
    eng.use_graph = False
    out = eng.train_step(ids, mask)
    assert out["optimizer_step"] is False and "grad_norm" not in out and "grad_clip_coef" not in out
    out = eng.train_step(ids2, mask2)
    assert out["optimizer_step"] is True and out["grad_clip_coef"].item() == 1.0
    want, got = _norm64(eng), out["grad_norm"].item()                             # over the MEAN of the two gradients
    print(f"grad_norm {got!r}, f64 norm over grads_by_parameter() {want!r}, rel {abs(got - want) / want:.3g}")
    assert want > 0 and abs(got - want) <= 1e-6 * want
    # a cycle whose first micro-batch gradient is not finite: the accumulator is poisoned, the final step stores nothing
    eng.forward_backward(ids, mask, compute_grads=True)
    eng.flat.grad[eng.flat.seg["enc.0.f1.w"][0] + 77] = float("inf")
    assert eng.finish_step() is False and eng.accum_pending == 1
    fl = eng.flat
    before = [t.clone() for t in (fl.master, fl.m, fl.v, fl.shadow, eng.E.data, eng.aux[0]["m"], eng.aux[0]["v"])]
    step0 = eng.step_count
    out = eng.train_step(ids2, mask2)
    torch.cuda.synchronize()
    assert out["optimizer_step"] is True and not math.isfinite(out["grad_norm"].item()) and out["grad_clip_coef"].item() == 0.0
    for a, b in zip(before, (fl.master, fl.m, fl.v, fl.shadow, eng.E.data, eng.aux[0]["m"], eng.aux[0]["v"])):
        assert torch.equal(_bits(a), _bits(b))
    assert eng.skipped_steps == 1 and eng.step_count == step0 + 1 and not bool(torch.isfinite(fl.acc).all())
    # the next cycle starts with a store: nothing of the poisoned one survives
    eng.train_step(ids, mask)
    out = eng.train_step(ids2, mask2)
    torch.cuda.synchronize()
    assert math.isfinite(out["grad_norm"].item()) and out["grad_clip_coef"].item() == 1.0
    assert bool(torch.isfinite(fl.acc).all()) and bool(torch.isfinite(eng.aux[0]["acc"]).all())
    assert not torch.equal(before[0], fl.master) and not torch.equal(before[4], eng.E.data)
    assert eng.skipped_steps == 1 and nnops.read_grad_guard(eng._guard)["skip"] == 0


def test_reset_pending_and_the_step_count_setter():
    from kvq import nnops
    from kvq.engine import TrainEngine
    ids, mask, _ = _batch(seed=9)
    eng = TrainEngine(_shelgon(torch.float32), lr=1e-3, grad_accum=3)
    eng.use_graph = False
    w0 = eng.flat.master.clone()
    eng.train_step(ids, mask)
    eng.train_step(ids, mask)
    assert eng.accum_pending == 2 and nnops.read_accum_state(eng._acc_state) == (2, 2)
    eng.reset_accumulation()                                                     # the started cycle is dropped
    assert eng.accum_pending == 0 and nnops.read_accum_state(eng._acc_state) == (2, 0)
    ran = [eng.train_step(ids, mask)["optimizer_step"] for _ in range(3)]
    assert ran == [False, False, True] and eng.step_count == 1 and not torch.equal(eng.flat.master, w0)
    want = eng.flat.grad.float() * 3 * torch.tensor(1 / 3, dtype=torch.float32, device="cuda")      # no dropout: three equal gradients
    a, b = eng.flat.ranges[0]
    torch.testing.assert_close(eng.flat.acc[a:b], want[a:b], rtol=1e-6, atol=0)   # only the new cycle's three, not five
    eng.train_step(ids, mask)
    eng.step_count = 5                                                           # a resumed run: five finished cycles
    assert eng.step_count == 5 and eng.accum_pending == 0
    assert nnops.read_accum_state(eng._acc_state) == (15, 0) and nnops.read_step_state(eng._state)[0] == 5


def test_combinations_that_are_not_built_are_refused(monkeypatch):
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    name = "kvq-bert-tiny-nodrop"

    def model(**vq_kw):
        torch.manual_seed(0)
        vq = VectorQuantizer(32, 128, 0.25, vq_codebook_init_values=torch.randn(32, 128), **vq_kw)
        return Shelgon(name, vq, name, None, compute_dtype=torch.bfloat16).cuda().train()

    with pytest.raises(KvqError, match="grad_accum.*revival"):
        TrainEngine(model(revive_after=2), grad_accum=2)
    with pytest.raises(KvqError, match="grad_accum.*EMA"):
        TrainEngine(model(ema_decay=0.99), grad_accum=2)
    monkeypatch.setenv("KVQ_DP_SINGLE_RANK", "1")
    with pytest.raises(KvqError, match="grad_accum.*data parallelism"):
        TrainEngine(model(), grad_accum=2)
    assert TrainEngine(model(), grad_accum=1).grad_accum == 1                    # off: nothing to refuse
    monkeypatch.delenv("KVQ_DP_SINGLE_RANK")
    monkeypatch.setenv("KVQ_VQ_REVIVE_AFTER", "3")
    with pytest.raises(KvqError, match="grad_accum.*revival"):
        TrainEngine(model(), grad_accum=2)
    monkeypatch.delenv("KVQ_VQ_REVIVE_AFTER")
    monkeypatch.setenv("KVQ_GRAD_ACCUM", "2")
    assert TrainEngine(model()).grad_accum == 2 and TrainEngine(model(), grad_accum=1).grad_accum == 1
    m = model()
    for bad in (0, -1, 2.5, True, "2"):                                          # refused before the model is touched
        with pytest.raises(KvqError, match="grad_accum"):
            TrainEngine(m, grad_accum=bad)
