"""TrainEngine.state_dict() / load_state_dict(): a resumed run continues bit for bit where the saved one
would have gone.  kvq-bert-tiny WITH dropout (a wrong seed offset shows), B = 16, S = 12, VectorQuantizer(32, 128, 0.25).

"Bits equal" = torch.equal on the raw words of flat.master / m / v (/ vmax), every aux p / m / v, the device structs, and every
step's returned losses.  The saved state always passes through torch.save and torch.load(weights_only=True); the resuming model
is built under another torch.manual_seed, so nothing it computes can come from its own initialisation."""
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

B, S = 16, 12
NAME = "kvq-bert-tiny"
LR = 1e-3


@pytest.fixture(autouse=True)
def _no_environment_switch(monkeypatch):
    for name in ("KVQ_GRAD_ACCUM", "KVQ_MAX_GRAD_NORM", "KVQ_VQ_REVIVE_AFTER", "KVQ_DP_SINGLE_RANK", "KVQ_FP8", "KVQ_FP8_BACKWARD",
                 "KVQ_FP8_W_PERIOD", "KVQ_FP8_ADAM", "KVQ_GRAPH"):
        monkeypatch.delenv(name, raising=False)


def _shelgon(dtype, seed=0, name=NAME, quantizer="vq", **vq_kw):
    from models.shelgon3.GumbelQuantizer import GumbelQuantizer
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(seed)
    if quantizer == "gumbel":
        vq = GumbelQuantizer(enc_out_size=128, n_embed=32, embedding_dim=128, temperature=1.0, kl_div_scale=5e-4, straight_through=True)
    else:
        vq = VectorQuantizer(32, 128, 0.25, vq_codebook_init_values=torch.randn(32, 128), **vq_kw)
        vq.materialize_min_encodings = False
    model = Shelgon(name, vq, name, None, compute_dtype=dtype).cuda()
    model.set_mode("full")
    return model.train()


def _bagon(dtype, seed=0, name=NAME):
    from models.bagon.Bagon import Bagon
    torch.manual_seed(seed)
    model = Bagon(name, name, True, compute_dtype=dtype).cuda()
    model.set_mode("full")
    return model.train()


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(3, S + 1, (B,), generator=g)
    ids = ids * (torch.arange(S)[None] < lens[:, None])
    noise = torch.randint(1000, 2000, (B, S), generator=g)
    dec = torch.where(torch.rand((B, S), generator=g) < 0.3, noise, ids) * (ids != 0)
    mask = (ids != 0).long()
    return ids.cuda(), mask.cuda(), dec.cuda()


def _raw(t):
    """The raw words of a tensor (NaNs and signed zeros compare as what they are)."""
    t = t.detach().contiguous().reshape(-1)
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _buffers(eng, shadow=False):
    """{name: tensor} of everything "bits equal" covers (live tensors, not copies)."""
    fl = eng.flat
    out = {"master": fl.master, "m": fl.m, "v": fl.v, "state": eng._state}
    if fl.vmax is not None:
        out["vmax"] = fl.vmax
    for i, a in enumerate(eng.aux):
        for k in ("p", "m", "v", "vmax"):
            if a.get(k) is not None:
                out[f"aux{i}.{k}"] = a[k].data
    if eng._acc_state is not None:
        out["acc_state"] = eng._acc_state
        if eng.accum_pending > 0:
            out["acc"] = fl.acc
            for i, a in enumerate(eng.aux):
                if "acc" in a:
                    out[f"aux{i}.acc"] = a["acc"]
    if eng._guard is not None:
        out["guard"] = eng._guard
    if eng.revive_after is not None:
        out["idle"], out["revive_counter"] = eng._rv_idle, eng._rv_counter
    if hasattr(eng, "E"):
        out["codebook"] = eng.E.data
    if eng.vq_ema:
        out["ema_n"], out["ema_m"] = eng.model.vector_quantizer.ema_n, eng.model.vector_quantizer.ema_m
    if eng.fp8:
        out.update(w8=eng._w8, w8_scale=eng._w8_scale, w8_amax=eng._w8_amax, a8_state=eng._a8_state)
        if eng.fp8_backward:
            out.update(g8_state=eng._g8_state, w8t=eng._w8t)
    if shadow:
        out["shadow"] = fl.shadow
    return out


def _snapshot(eng, shadow=False):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in _buffers(eng, shadow).items()}


def _assert_bits_equal(a, b, what):
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    bad = [k for k in a if a[k].shape != b[k].shape or not torch.equal(_raw(a[k]), _raw(b[k]))]
    assert not bad, f"{what}: bits differ in {bad}"


def _losses(out):
    return {k: _raw(out[k]).clone() for k in ("loss_recon", "loss_vq", "acc", "perplexity", "grad_norm", "codes_revived")
            if out.get(k) is not None}


def _step(eng, i, poison=False):
    """Training step number i (1-based) of the fixed batch sequence.  poison: backward, one gradient element set to NaN, then the
    rest of the step (the way tests/test_grad_guard_engine_gpu.py makes a non-finite step)."""
    ids, mask, dec = _batch(100 + i)
    kw = {} if eng.has_vq else dict(dec_ids=dec, dec_mask=mask)
    if poison:
        out = eng.forward_backward(ids, mask, compute_grads=True, **kw)
        eng.flat.grad[eng.flat.seg["enc.0.f1.w"][0] + 77] = float("nan")
        eng.finish_step()
        return out
    return eng.train_step(ids, mask, **kw)


def _through_a_file(obj, path=None):
    """torch.save, then torch.load(weights_only=True): what comes back is what a resumed process reads."""
    f = path if path is not None else io.BytesIO()
    torch.save(obj, f)
    if path is None:
        f.seek(0)
    return torch.load(f, weights_only=True)


def _engine(make, use_graph=True, seed=0, **kw):
    from kvq.engine import TrainEngine
    eng = TrainEngine(make(seed), lr=LR, **kw)
    eng.use_graph = use_graph
    return eng


def _round_trip(make, eng_kw, tmp_path, save_at=4, total=8, use_graph=True, poison_at=None, at_save=None):
    """Run A trains `total` steps.  Run B trains `save_at`, its state_dict() + model.state_dict() pass through a file, a FRESH model
    built under another torch.manual_seed and a fresh engine load them.  A (replaying its graphs by then) and the resumed engine
    (eager for its first calls, then capturing) are stepped side by side: bits equal after every step.  Returns (A, resumed, state,
    per-step outputs of A, of the resumed engine)."""
    a = _engine(make, use_graph, **eng_kw)
    outs_a = {i: _step(a, i, poison=i == poison_at) for i in range(1, save_at + 1)}
    at4 = _snapshot(a, shadow=True)
    b = _engine(make, use_graph, **eng_kw)
    for i in range(1, save_at + 1):
        _step(b, i, poison=i == poison_at)
    if at_save is not None:
        at_save(b)
    blob = _through_a_file({"engine": b.state_dict(), "model": b.model.state_dict()}, str(tmp_path / "state.pth"))
    _assert_bits_equal(_snapshot(b, shadow=True), at4, "two runs of the same steps (and state_dict() wrote nothing)")
    del b
    c = _engine(make, use_graph, seed=4321, **eng_kw)
    assert not torch.equal(c.flat.master, a.flat.master)
    c.model.load_state_dict(blob["model"])
    c.load_state_dict(blob["engine"])
    _assert_bits_equal(_snapshot(c, shadow=True), at4, f"straight after the load (step {save_at}), shadow included")
    assert c.step_count == a.step_count and c.accum_pending == a.accum_pending
    outs_c = {}
    for i in range(save_at + 1, total + 1):
        outs_a[i], outs_c[i] = _step(a, i), _step(c, i)
        la, lc = _losses(outs_a[i]), _losses(outs_c[i])
        assert set(la) == set(lc) and all(torch.equal(la[k], lc[k]) for k in la), f"step {i}: returned losses differ"
        assert outs_a[i].get("optimizer_step") == outs_c[i].get("optimizer_step")
        _assert_bits_equal(_snapshot(c), _snapshot(a), f"after step {i}")
    if use_graph:
        assert a._graphs and c._graphs            # A replayed steps save_at+1 ..., the resumed engine ran two eagerly and captured
    return a, c, blob["engine"], outs_a, outs_c


# ---- 1. round trip -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["shelgon", "bagon"])
def test_round_trip_continues_bit_for_bit(kind, dtype, use_graph, tmp_path):
    make = (lambda seed: _shelgon(dtype, seed)) if kind == "shelgon" else (lambda seed: _bagon(dtype, seed))
    a, c, state, _, _ = _round_trip(make, {}, tmp_path, use_graph=use_graph)
    assert a.step_count == c.step_count == 8
    assert state["format"] == 1 and state["host"] == {"step": 4, "accum_pending": 0, "grads_are_mean": False}
    assert [e[0] for e in state["fingerprint"]["layout"]] == list(a.flat.seg) and state["fingerprint"]["flat_n"] == a.flat.n
    assert state["flat"]["master"].numel() == a.flat.n and not state["flat"]["master"].is_cuda          # whole, padding included
    assert set(state["flat"]) == {"master", "m", "v"} and "fp8" not in state


# ---- 2. a snapshot disturbs nothing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_a_snapshot_disturbs_nothing(use_graph):
    make = lambda seed: _shelgon(torch.bfloat16, seed)
    runs = []
    for snap in (False, True):
        eng = _engine(make, use_graph)
        outs = []
        for i in range(1, 7):
            outs.append(_losses(_step(eng, i)))
            if snap and i == 3:
                st = eng.state_dict()
                assert st["host"]["step"] == 3
        runs.append((_snapshot(eng, shadow=True), outs))
    _assert_bits_equal(runs[0][0], runs[1][0], "six steps with a state_dict() after the third")
    for i, (x, y) in enumerate(zip(runs[0][1], runs[1][1])):
        assert all(torch.equal(x[k], y[k]) for k in x), f"step {i + 1}: losses"


def test_an_engine_that_never_trained_saves_and_loads():
    """Before the first step there are no moments: the state holds none, and loading it resets an engine that has trained."""
    make = lambda seed: _shelgon(torch.bfloat16, seed)
    fresh = _engine(make, False)
    st = _through_a_file(fresh.state_dict())
    assert set(st["flat"]) == {"master"} and not fresh.flat.optimizer_state_allocated()
    ref = [_losses(_step(fresh, i)) for i in (1, 2)]
    eng = _engine(make, False, seed=9)
    for i in (1, 2, 3):
        _step(eng, i)
    eng.load_state_dict(st)
    assert eng.step_count == 0 and float(eng.flat.m.abs().max()) == 0.0 and float(eng.flat.v.abs().max()) == 0.0
    got = [_losses(_step(eng, i)) for i in (1, 2)]
    for x, y in zip(ref, got):
        assert all(torch.equal(x[k], y[k]) for k in x)
    _assert_bits_equal(_snapshot(eng), _snapshot(fresh), "two steps from a step-0 state")


# ---- 3. in place -----------------------------------------------------------------------------------------------------------------------
def test_load_is_in_place_and_the_graphs_keep_replaying():
    make = lambda seed: _shelgon(torch.bfloat16, seed)
    eng = _engine(make, True)
    for i in range(1, 5):
        _step(eng, i)
    assert eng._graphs                                           # replaying by step 3
    state = _through_a_file({"engine": eng.state_dict(), "model": eng.model.state_dict()})
    first = []
    for i in range(5, 9):
        first.append((_losses(_step(eng, i)), _snapshot(eng)))
    ptrs = {k: v.data_ptr() for k, v in _buffers(eng, shadow=True).items()}
    ptrs["grad"] = eng.flat.grad.data_ptr()
    graphs = dict(eng._graphs)
    eng.model.load_state_dict(state["model"])
    eng.load_state_dict(state["engine"])
    assert {k: v.data_ptr() for k, v in _buffers(eng, shadow=True).items()} == {k: v for k, v in ptrs.items() if k != "grad"}
    assert eng.flat.grad.data_ptr() == ptrs["grad"]
    assert eng._graphs == graphs and all(eng._graphs[k] is graphs[k] for k in graphs)          # not enlarged, not rebuilt
    assert eng.step_count == 4
    for n, i in enumerate(range(5, 9)):
        losses = _losses(_step(eng, i))                          # a replay: no new chain
        assert all(torch.equal(losses[k], first[n][0][k]) for k in losses), f"step {i}: losses"
        _assert_bits_equal(_snapshot(eng), first[n][1], f"step {i}, run again after the load")
    assert eng._graphs == graphs


# ---- 4. options ------------------------------------------------------------------------------------------------------------------------
def test_option_gradient_guard_with_a_skipped_step(tmp_path):
    make = lambda seed: _shelgon(torch.bfloat16, seed)
    seen = {}
    a, c, state, _, _ = _round_trip(make, dict(max_grad_norm=1.0), tmp_path, use_graph=False, poison_at=3,
                                    at_save=lambda b: seen.update(skipped=b.skipped_steps))
    assert seen["skipped"] >= 1                                  # the condition: a step was skipped before the save
    assert c.skipped_steps == a.skipped_steps >= 1 and "guard" in state["structs"]


@pytest.mark.parametrize("save_at,pending", [(5, 2), (6, 0)])
def test_option_gradient_accumulation(tmp_path, save_at, pending):
    make = lambda seed: _shelgon(torch.bfloat16, seed)
    seen = {}
    a, c, state, outs_a, outs_c = _round_trip(make, dict(grad_accum=3), tmp_path, save_at=save_at, total=10,
                                              at_save=lambda b: seen.update(pending=b.accum_pending))
    assert seen["pending"] == pending == state["host"]["accum_pending"]
    has_acc = "acc" in state["flat"], any("acc" in d for d in state["aux"])
    if pending:
        assert has_acc == (True, True)                           # the accumulator of the open cycle travels
        assert outs_c[save_at + 1]["optimizer_step"] is True     # ... and the first call after the load closes that cycle
    else:
        assert has_acc == (False, False)                         # between two cycles there is nothing to carry
        assert outs_c[save_at + 1]["optimizer_step"] is False
    assert c.step_count == a.step_count == 3 and "acc_state" in state["structs"]


def test_option_codebook_revival(tmp_path):
    make = lambda seed: _shelgon(torch.bfloat16, seed, revive_after=2)
    seen = {}
    a, c, state, _, _ = _round_trip(make, {}, tmp_path, at_save=lambda b: seen.update(revived=b.revived_codes))
    print("codes revived before the save:", seen["revived"], "at the end:", a.revived_codes)
    assert seen["revived"] >= 1 and a.revived_codes > seen["revived"]          # the condition: revivals on both sides of the save
    assert c.revived_codes == a.revived_codes and torch.equal(c.code_idle, a.code_idle)
    assert state["structs"]["revive_idle"].dtype == torch.int32 and state["structs"]["revive_counter"].tolist()[1] == seen["revived"]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_option_ema_codebook(tmp_path, use_graph):
    """(With graphs A captures at step 3 and the resumed engine at step 7: capturing a step must leave the EMA statistics alone.)"""
    make = lambda seed: _shelgon(torch.bfloat16, seed, ema_decay=0.99)
    a, c, state, _, _ = _round_trip(make, {}, tmp_path, use_graph=use_graph)
    vq = a.model.vector_quantizer
    assert a.vq_ema and not a.E.requires_grad and not torch.equal(vq.ema_n, torch.ones_like(vq.ema_n))      # the statistics moved
    assert not torch.equal(state["structs"]["ema_n"], vq.ema_n.cpu())                                       # ... on both sides of the save


def test_ema_codebook_replayed_steps_equal_eager_steps():
    """The invariant the resume contract rests on, for the EMA codebook: its update is an eager launch between the step's graphs,
    and the capture of a step (which runs every such launch once, on buffers no graph has written yet) is no training step."""
    runs = []
    for use_graph in (False, True):
        eng = _engine(lambda seed: _shelgon(torch.bfloat16, seed, ema_decay=0.99), use_graph)
        outs = [_losses(_step(eng, i)) for i in range(1, 6)]
        assert bool(eng._graphs) == use_graph
        runs.append((_snapshot(eng, shadow=True), outs, eng.E.data.clone()))
    _assert_bits_equal(runs[0][0], runs[1][0], "five steps, eager against replayed")
    assert torch.equal(runs[0][2], runs[1][2])
    for i, (x, y) in enumerate(zip(runs[0][1], runs[1][1])):
        assert all(torch.equal(x[k], y[k]) for k in x), f"step {i + 1}: losses"


def test_option_amsgrad(tmp_path):
    make = lambda seed: _shelgon(torch.bfloat16, seed)
    a, c, state, _, _ = _round_trip(make, dict(amsgrad=True), tmp_path)
    assert "vmax" in state["flat"] and float(state["flat"]["vmax"].max()) > 0 and all("vmax" in d for d in state["aux"])


def test_option_milestones_on_both_sides_of_the_save(tmp_path):
    from kvq import nnops
    make = lambda seed: _shelgon(torch.bfloat16, seed)
    seen = {}
    a, c, state, _, _ = _round_trip(make, dict(milestones=[3, 6]), tmp_path,
                                    at_save=lambda b: seen.update(lr=nnops.read_step_state(b._state)[1]))
    lr_end = nnops.read_step_state(c._state)[1]
    print("lr at the save:", seen["lr"], "at the end:", lr_end)
    assert abs(seen["lr"] - LR * 0.1) <= 1e-6 * LR and abs(lr_end - LR * 0.01) <= 1e-7 * LR      # one milestone before, one after


def test_option_gumbel_quantiser(tmp_path):
    make = lambda seed: _shelgon(torch.bfloat16, seed, quantizer="gumbel")
    a, c, state, outs_a, _ = _round_trip(make, {}, tmp_path)
    assert a.vq_kind == "GumbelQuantizer" and len(a.aux) == 3 and len(state["aux"]) == 3
    assert len({int(_losses(outs_a[i])["loss_vq"][0]) for i in outs_a}) == len(outs_a)      # every step drew its own noise


# ---- 5. fp8 ------------------------------------------------------------------------------------------------------------------------------
def test_fp8_forward_and_backward_across_a_weight_scale_refresh():
    """The model and batch of tests/test_fp8_backward_gpu.py (bert-base widths, 2 + 2 layers, 256 token rows).  Saved at step 5 --
    behind the calibration step, inside a weight-scale period of 16 --, resumed through step 18, across the refresh at step 16.
    Run A is also the run that saves (test 2 covers that a snapshot disturbs nothing): one engine of this size less."""
    from dsentences.synthetic import random_token_batch
    from kvq.engine import TrainEngine
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer

    def build(seed):
        torch.manual_seed(seed)
        vq = VectorQuantizer(512, 768, 0.25, vq_codebook_init_values=torch.randn(512, 768))
        vq.materialize_min_encodings = False
        return Shelgon("kvq-bert-base-2l", vq, "kvq-bert-base-2l", None, compute_dtype=torch.bfloat16).cuda().train()

    ids, mask = (t.cuda() for t in random_token_batch(8, 32, torch.Generator().manual_seed(0)))
    kw = dict(lr=2e-4, fp8_forward=True, fp8_backward=True)
    a = TrainEngine(build(1), **kw)
    assert a._w8_period == 16
    for _ in range(5):
        a.train_step(ids, mask)
    assert a._g8_ready and a._g8_live and a.fp8_bwd_launches > 0
    blob = _through_a_file({"engine": a.state_dict(), "model": a.model.state_dict()})
    st = blob["engine"]
    assert st["fp8"]["g8_ready"] is True and st["fp8"]["g8_live"] == sorted(a._g8_live) and "w8t" not in st["fp8"]
    assert set(st["fp8"]) == {"w8", "w8_amax", "w8_scale", "a8_state", "g8_state", "g8_ready", "g8_live"}
    scale5 = a._w8_scale.clone()
    c = TrainEngine(build(77), **kw)
    c.model.load_state_dict(blob["model"])
    c.load_state_dict(st)
    del blob, st
    assert c._g8_ready and c._g8_live == a._g8_live
    _assert_bits_equal(_snapshot(c, shadow=True), _snapshot(a, shadow=True), "straight after the load (step 5)")
    for i in range(6, 19):
        oa, oc = a.train_step(ids, mask), c.train_step(ids, mask)
        assert c.fp8_bwd_launches == a.fp8_bwd_launches > 0, i    # the resumed engine never calibrates again
        la, lc = _losses(oa), _losses(oc)
        assert all(torch.equal(la[k], lc[k]) for k in la), f"step {i}: losses"
        torch.cuda.synchronize()
        bad = [k for k, v in _buffers(a).items() if not torch.equal(_raw(v), _raw(_buffers(c)[k]))]
        assert not bad, f"after step {i}: bits differ in {bad}"
    assert a.step_count == c.step_count == 18 and not torch.equal(scale5, c._w8_scale)      # the refresh at step 16 happened


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def saved_state():
    import os
    for name in ("KVQ_GRAD_ACCUM", "KVQ_MAX_GRAD_NORM", "KVQ_VQ_REVIVE_AFTER", "KVQ_FP8", "KVQ_FP8_BACKWARD"):
        os.environ.pop(name, None)
    eng = _engine(lambda seed: _shelgon(torch.bfloat16, seed), False)
    for i in (1, 2):
        _step(eng, i)
    return _through_a_file(eng.state_dict())


@pytest.mark.parametrize("case,key", [("grad_accum", "fingerprint.grad_accum"), ("seed", "fingerprint.seed"), ("lr", "fingerprint.lr"),
                                      ("dtype", "fingerprint.dtype"), ("layers", "fingerprint.layout"), ("format", "format"),
                                      ("missing", "flat.v"), ("missing_struct", "structs.state"), ("version", "kvq_version")])
def test_refusals_name_the_key_and_write_nothing(saved_state, case, key, monkeypatch):
    import copy
    from kvq._ffi import KvqError
    from models.bagon import Bagon as bagon_module
    state = copy.deepcopy(saved_state)
    dtype, name, kw = torch.bfloat16, NAME, {}
    if case == "grad_accum":
        kw = dict(grad_accum=2)
    elif case == "seed":
        kw = dict(seed=7)
    elif case == "dtype":
        dtype = torch.float32
    elif case == "layers":
        cfg = dict(bagon_module.LOCAL_BERT_CONFIGS[NAME], num_hidden_layers=1)
        monkeypatch.setitem(bagon_module.LOCAL_BERT_CONFIGS, "kvq-bert-tiny-1l", cfg)
        name = "kvq-bert-tiny-1l"
    elif case == "format":
        state["format"] = 99
    elif case == "missing":
        del state["flat"]["v"]
    elif case == "missing_struct":
        del state["structs"]["state"]
    elif case == "version":
        state["kvq_version"] += 1
    from kvq.engine import TrainEngine
    eng = TrainEngine(_shelgon(dtype, 5, name=name), lr=2e-3 if case == "lr" else LR, **kw)
    eng.use_graph = False
    _step(eng, 1)
    before = _snapshot(eng, shadow=True)
    host = (eng.step_count, eng.accum_pending, eng._param_versions)
    with pytest.raises(KvqError) as err:
        eng.load_state_dict(state)
    print(err.value)
    assert key in str(err.value)
    if case == "lr":
        assert "0.001" in str(err.value) and "0.002" in str(err.value)          # both values
    _assert_bits_equal(_snapshot(eng, shadow=True), before, "a refused load")
    assert (eng.step_count, eng.accum_pending, eng._param_versions) == host
    _step(eng, 2)                                                # ... and the engine trains on
