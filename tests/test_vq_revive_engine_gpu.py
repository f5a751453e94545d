"""Codebook revival inside the TrainEngine step (VectorQuantizer(revive_after=...)) against the numpy
restatement (tests/_revive_ref.py): idle counters, revived rows, moments and counters after every step; the eager step against the
hipGraph replay; the multi-codebook and EMA quantisers; an engine without the option; the module path.

kvq-bert-tiny, K = 64 codes and 4 x 8 = 32 tokens: at most 32 codes win a token in a step, so at least 32 are dead from step
revive_after on -- revival is certain, not hoped for."""
import numpy as np
import pytest
import torch

import _revive_ref as R

pytestmark = pytest.mark.gpu

B, S, K, H = 4, 8, 64, 128
NAME = "kvq-bert-tiny"


@pytest.fixture(autouse=True)
def _no_environment_switch(monkeypatch):
    monkeypatch.delenv("KVQ_VQ_REVIVE_AFTER", raising=False)


def _codebook():
    return torch.randn(K, H, generator=torch.Generator().manual_seed(5))


def _shelgon(dtype, kind="single", revive_after=None, ema=None):
    from models.shelgon3.MultiVectorQuantizer import MultiVectorQuantizer
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(0)
    if kind == "multi":
        vq = MultiVectorQuantizer(2, K, H, 0.25, ema_decay=ema, revive_after=revive_after)
    else:
        vq = VectorQuantizer(K, H, 0.25, vq_codebook_init_values=_codebook(), ema_decay=ema, revive_after=revive_after)
        vq.materialize_min_encodings = False
    model = Shelgon(NAME, vq, NAME, None, compute_dtype=dtype).cuda()
    model.set_mode("full")
    return model


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(3, S + 1, (B,), generator=g)
    ids = ids * (torch.arange(S)[None] < lens[:, None])
    return ids.cuda(), (ids != 0).long().cuda()


def _np(t):
    return t.detach().float().cpu().numpy()


def _drive(eng, steps, T, same_batch=False, check_donors=True):
    """Run `steps` training steps with lr = 0 and drive the restatement with each step's indices, the engine's seed and the donor
    source the select kernel read.  Returns one record per step: what the restatement predicts and what the engine holds."""
    G, Kk, D = eng.G, eng.K, eng.Dg
    eng.revive_keep_donors = True
    idle = np.zeros((G, Kk), np.int32)
    E = _np(eng.E).reshape(G, Kk, D)
    total, recs = 0, []
    for s in range(steps):
        ids, mask = _batch(1 if same_batch else 10 + s)
        out = eng.train_step(ids, mask)
        torch.cuda.synchronize()
        donors = eng.revive_donors
        if check_donors:                # the donor source is the encoder output of this batch, to the dtype's rounding
            z = eng.encode(ids, mask, quantize=False)["z"].reshape(B * S, H)
            zg = eng.model.vector_quantizer.split(z) if G > 1 else z.view(1, B * S, H)
            eps = torch.finfo(z.dtype).eps
            assert torch.allclose(donors.float(), zg.float(), rtol=2 * eps, atol=2 * eps * float(zg.float().abs().max())), s
        idx = out["indices"].reshape(B * S, G).t().contiguous().cpu().numpy()
        used = R.usage_flags(idx, Kk)
        seed = eng._step_seed + s                                    # the device step count BEFORE this step's advance
        idle_sel, dead, rows, _owner, token = R.select([_np(donors)], used, idle, T, seed)
        E_before = E
        idle, E, (last, total), _ = R.apply(rows, dead, idle_sel, E, (0, total))
        recs.append(dict(step=s, out=out, idx=idx, donors=donors.clone(), seed=seed, dead=dead, rows=rows, token=token, idle=idle, E=E,
                         E_before=E_before, last=last, total=total,
                         eng_idle=eng.code_idle.cpu().numpy().copy(), eng_E=_np(eng.E).reshape(G, Kk, D).copy(),
                         eng_revived=eng.revived_codes, eng_last=int(out["codes_revived"].item())))
    return recs


@pytest.fixture(scope="module")
def single_f32():
    """(a) in f32, computed once: the module-path test (e) replays the same inputs."""
    import os
    from kvq.engine import TrainEngine
    os.environ.pop("KVQ_VQ_REVIVE_AFTER", None)
    model = _shelgon(torch.float32, revive_after=2).eval()
    eng = TrainEngine(model, lr=0.0)
    recs = _drive(eng, 5, 2)
    return eng, recs


def _check_adam_run(eng, recs, T):
    a = eng.aux[0]
    assert a["p"] is eng.E
    revived_any = 0
    for r in recs:
        s = r["step"]
        assert np.array_equal(r["eng_idle"], r["idle"]), f"step {s}: code_idle"
        assert r["eng_last"] == r["last"] and r["eng_revived"] == r["total"], (s, r["eng_last"], r["last"], r["eng_revived"], r["total"])
        dead = r["dead"]
        assert np.array_equal(R.bits(r["eng_E"][dead]), R.bits(r["rows"][dead])), f"step {s}: revived rows"
        assert np.array_equal(R.bits(r["eng_E"][~dead]), R.bits(r["E_before"][~dead])), f"step {s}: other rows keep their bits (lr = 0)"
        if s + 1 < T:
            assert r["last"] == 0                                                       # nothing can be dead before step T
        elif s + 1 == T:
            assert r["last"] >= eng.G * (K - B * S)                                     # at most B * S codes per codebook ever won a token
        revived_any += r["last"]
    assert revived_any > 0
    dead = torch.from_numpy(recs[-1]["dead"]).cuda().view(-1)                           # the last step's revived rows: moments restarted
    assert not a["m"][dead].any() and not a["v"][dead].any()
    assert a["m"].abs().sum() > 0                                                       # (while the codes in use do have moments)
    o = recs[-1]["out"]["codes_revived"]
    assert o.is_cuda and o.numel() == 1 and o.dtype == torch.int64


def test_revival_follows_the_restatement_f32(single_f32):
    eng, recs = single_f32
    assert eng._graphs, "steps 3.. were replayed from the captured step"
    _check_adam_run(eng, recs, 2)


def test_revival_follows_the_restatement_bf16():
    from kvq.engine import TrainEngine
    model = _shelgon(torch.bfloat16, revive_after=2).eval()
    eng = TrainEngine(model, lr=0.0)
    _check_adam_run(eng, _drive(eng, 5, 2), 2)
    assert eng.model.vector_quantizer.code_idle.data_ptr() == eng.code_idle.data_ptr()     # the module's buffer IS the engine's state


def test_eager_equals_replay_and_the_graphs_hold_kernels_only():
    """(b) lr = 1e-3, dropout on, 6 steps: eager against replay, bit for bit; no memset / memcpy node in the replayed graphs."""
    from kvq.engine import TrainEngine
    runs = []
    for use_graph in (False, True):
        eng = TrainEngine(_shelgon(torch.bfloat16, revive_after=2).train(), lr=1e-3)
        eng.use_graph = use_graph
        counts = []
        for s in range(6):
            ids, mask = _batch(20 + s)
            counts.append(eng.train_step(ids, mask)["codes_revived"])
        torch.cuda.synchronize()
        assert bool(eng._graphs) == use_graph and eng.step_count == 6
        if use_graph:
            census = next(iter(eng._graphs.values())).node_census()
            print("graphs of the step chain with revive_after:", census)
            for c in census:
                assert c["memset"] == 0 and c["memcpy"] == 0 and c["other"] == 0, census
        a = eng.aux[0]
        runs.append(dict(E=eng.E.detach().clone(), idle=eng.code_idle.clone(), m=a["m"].clone(), v=a["v"].clone(),
                         counter=eng._rv_counter.clone(), counts=torch.stack(counts), master=eng.flat.master.clone()))
    eager, replay = runs
    print("codes revived per step:", eager["counts"].tolist(), "replayed:", replay["counts"].tolist(), "counter", eager["counter"].tolist())
    for k in eager:
        assert torch.equal(eager[k], replay[k]), k
    assert eager["counts"].sum().item() == eager["counter"][1].item() > 0


@pytest.mark.parametrize("kind,ema", [("multi", None), ("single", 0.99), ("multi", 0.99)], ids=["multi", "ema", "multi-ema"])
def test_multi_codebook_and_ema(kind, ema):
    """(c) the same drive with two codebooks on two slices and with the EMA codebook: revived rows, ema_n == 1, ema_m rows.  The
    EMA arms run every step eagerly: with EMA every codebook row moves in every step, so only the revived rows are predictable."""
    from kvq.engine import TrainEngine
    model = _shelgon(torch.bfloat16, kind=kind, revive_after=2, ema=ema).eval()
    eng = TrainEngine(model, lr=0.0)
    if ema is not None:
        eng.use_graph = False
    G = 2 if kind == "multi" else 1
    assert eng.G == G and eng.code_idle.shape == (G, K)
    recs = _drive(eng, 5, 2)
    if ema is None:
        _check_adam_run(eng, recs, 2)
        return
    vq = model.vector_quantizer
    for r in recs:
        s, dead = r["step"], r["dead"]
        assert np.array_equal(r["eng_idle"], r["idle"]), f"step {s}: code_idle"
        assert r["eng_last"] == r["last"] and r["eng_revived"] == r["total"]
        assert np.array_equal(R.bits(r["eng_E"][dead]), R.bits(r["rows"][dead])), f"step {s}: revived rows"
    assert recs[-1]["total"] > 0
    dead = recs[-1]["dead"]
    ema_n, ema_m = _np(vq.ema_n).reshape(G, K), _np(vq.ema_m).reshape(G, K, -1)
    assert (ema_n[dead] == 1.0).all() and not (ema_n[~dead] == 1.0).all()
    assert np.array_equal(R.bits(ema_m[dead]), R.bits(recs[-1]["rows"][dead]))


def test_an_engine_without_the_option_and_gumbel(monkeypatch):
    """(d)"""
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    from models.shelgon3.GumbelQuantizer import GumbelQuantizer
    from models.shelgon3.Shelgon import Shelgon
    model = _shelgon(torch.bfloat16).train()
    eng = TrainEngine(model, lr=1e-3)
    ids, mask = _batch(3)
    out = eng.train_step(ids, mask)
    assert "codes_revived" not in out and eng.revive_after is None and eng.code_idle is None and eng.revived_codes == 0
    assert not hasattr(eng, "_rv_idle") and not hasattr(eng, "_rv_rows") and list(model.vector_quantizer.buffers()) == []
    # the environment switch: the state is the engine's own, the module stays as it was
    monkeypatch.setenv("KVQ_VQ_REVIVE_AFTER", "1")
    model = _shelgon(torch.bfloat16).train()
    eng = TrainEngine(model, lr=1e-3)
    out = eng.train_step(ids, mask)
    assert eng.revive_after == 1 and out["codes_revived"].item() >= K - B * S and eng.code_idle.shape == (1, K)
    assert list(model.vector_quantizer.buffers()) == []
    for bad in ("0", "soon", "1.5"):
        monkeypatch.setenv("KVQ_VQ_REVIVE_AFTER", bad)
        with pytest.raises(KvqError, match="revive_after"):
            TrainEngine(_shelgon(torch.bfloat16), lr=1e-3)
    # forward-only calls neither revive nor advance idle
    monkeypatch.delenv("KVQ_VQ_REVIVE_AFTER")
    model = _shelgon(torch.bfloat16, revive_after=1).eval()
    eng = TrainEngine(model, lr=1e-3)
    eng.forward_logits(ids, mask)
    eng.encode(ids, mask)
    eng.eval_step(ids, mask)
    torch.cuda.synchronize()
    assert not eng.code_idle.any() and eng.revived_codes == 0
    # Gumbel: refused
    monkeypatch.setenv("KVQ_VQ_REVIVE_AFTER", "3")
    torch.manual_seed(0)
    gq = GumbelQuantizer(enc_out_size=H, n_embed=K, embedding_dim=H, temperature=1.0, kl_div_scale=5e-4, straight_through=True)
    gmodel = Shelgon(NAME, gq, NAME, None, compute_dtype=torch.bfloat16).cuda()
    with pytest.raises(KvqError, match="GumbelQuantizer"):
        TrainEngine(gmodel, lr=1e-3)


def test_module_path_gives_the_engines_bits(single_f32):
    """(e) VectorQuantizer.revive() fed the engine's inputs (donor source, indices, seed) step by step: the same idle counters,
    codebook bits and counts (lr = 0: the engine's codebook moves by revival alone)."""
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    _eng, recs = single_f32
    vq = VectorQuantizer(K, H, 0.25, vq_codebook_init_values=_codebook(), revive_after=2).cuda()
    epoch0 = getattr(vq, "codebook_epoch", 0)
    total = 0
    for r in recs:
        n = vq.revive(r["donors"].view(B * S, H), torch.from_numpy(r["idx"]).cuda().view(-1), seed=r["seed"])
        assert n.is_cuda and n.item() == r["eng_last"]
        total += n.item()
        assert np.array_equal(vq.code_idle.cpu().numpy().reshape(1, K), r["eng_idle"])
        assert np.array_equal(R.bits(_np(vq.embedding.weight).reshape(1, K, H)), R.bits(r["eng_E"]))
    assert vq.codebook_epoch == epoch0 + len(recs) and total == recs[-1]["eng_revived"] > 0
