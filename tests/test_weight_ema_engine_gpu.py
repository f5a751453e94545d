"""TrainEngine(weight_ema=decay): the average the step keeps is the restatement's recurrence over the weights
the optimiser left, eager and replayed steps agree bit for bit, the option off launches nothing, evaluation inside
weight_ema_applied() IS evaluation of the averaged weights and leaving the scope restores every bit, a skipped step and the
micro-steps of an accumulation cycle do not move the average, and a resumed run continues it.  kvq-bert-tiny WITH dropout, B = 16,
S = 12, VectorQuantizer(32, 128, 0.25); "bits equal" = equality of the raw words."""
import io

import numpy as np
import pytest
import torch

import _weight_ema_ref as R

pytestmark = pytest.mark.gpu

B, S = 16, 12
NAME = "kvq-bert-tiny"
LR = 1e-3
DECAY = 0.999
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
# today's fingerprint: an engine without the option must keep exactly these keys
FINGERPRINT_KEYS = {"layout", "flat_n", "dtype", "lr", "betas", "eps", "weight_decay", "amsgrad", "milestones", "gamma", "w_recon", "w_vq",
                    "seed", "grad_accum", "max_grad_norm", "revive_after", "vq_kind", "G", "K", "Dg", "vq_ema", "aux", "fp8", "fp8_backward",
                    "w8_period", "w8_in_adam", "w8_keys", "world"}


@pytest.fixture(autouse=True)
def _no_environment_switch(monkeypatch):
    for name in ("KVQ_WEIGHT_EMA", "KVQ_GRAD_ACCUM", "KVQ_MAX_GRAD_NORM", "KVQ_VQ_REVIVE_AFTER", "KVQ_DP_SINGLE_RANK", "KVQ_FP8",
                 "KVQ_FP8_BACKWARD", "KVQ_GRAPH"):
        monkeypatch.delenv(name, raising=False)


def _shelgon(dtype, seed=0, mode="full"):
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(seed)
    vq = VectorQuantizer(32, 128, 0.25, vq_codebook_init_values=torch.randn(32, 128))
    vq.materialize_min_encodings = False
    model = Shelgon(NAME, vq, NAME, None, compute_dtype=dtype).cuda()
    model.set_mode(mode)
    return model.train()


def _engine(dtype, use_graph=True, seed=0, mode="full", **kw):
    from kvq.engine import TrainEngine
    eng = TrainEngine(_shelgon(dtype, seed, mode), lr=LR, **kw)
    eng.use_graph = use_graph
    return eng


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(3, S + 1, (B,), generator=g)
    ids = ids * (torch.arange(S)[None] < lens[:, None])
    return ids.cuda(), (ids != 0).long().cuda()


def _step(eng, i):
    return eng.train_step(*_batch(100 + i))


def _raw(t):
    t = t.detach().contiguous().reshape(-1)
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _np(t):
    return t.detach().float().cpu().numpy() if t.dtype != torch.float32 else t.detach().cpu().numpy()


def _averaged(eng):
    """{name: (parameters, average)} of everything the option averages, as live views: the trainable ranges, the aux parameters."""
    fl = eng.flat
    out = {f"range[{a}:{b}]": (fl.master[a:b], fl.ema[a:b]) for (a, b) in fl.ranges}
    for i, x in enumerate(eng.aux):
        if x["p"].requires_grad:
            out[f"aux{i}"] = (x["p"].data.view(-1), x["ema"].view(-1))
    return out


def _snapshot(eng, shadow=True):
    torch.cuda.synchronize()
    fl = eng.flat
    out = {"master": fl.master, "m": fl.m, "v": fl.v, "state": eng._state, "codebook": eng.E.data}
    if shadow:
        out["shadow"] = fl.shadow
    for i, a in enumerate(eng.aux):
        out.update({f"aux{i}.{k}": a[k] for k in ("m", "v")})
    if eng.weight_ema is not None:
        out["wema_state"] = eng._wema_state
        for k, (_, ema) in _averaged(eng).items():          # (outside the ranges flat.ema is memory nobody wrote: not compared)
            out["ema." + k] = ema
    if eng._guard is not None:
        out["guard"] = eng._guard
    if eng._acc_state is not None:
        out["acc_state"] = eng._acc_state
    return {k: v.detach().clone() for k, v in out.items()}


def _assert_bits_equal(a, b, what):
    assert set(a) == set(b), (what, sorted(set(a) ^ set(b)))
    bad = [k for k in a if a[k].shape != b[k].shape or not torch.equal(_raw(a[k]), _raw(b[k]))]
    assert not bad, f"{what}: bits differ in {bad}"


def _losses(out):
    return {k: _raw(out[k]).clone() for k in ("loss_recon", "loss_vq", "acc", "perplexity", "grad_norm", "weight_ema_decay", "indices",
                                               "recon_ids") if out.get(k) is not None}


def _assert_same_losses(x, y, what):
    lx, ly = _losses(x), _losses(y)
    assert set(lx) == set(ly) and all(torch.equal(lx[k], ly[k]) for k in lx), f"{what}: returned values differ"


def _through_a_file(obj):
    f = io.BytesIO()
    torch.save(obj, f)
    f.seek(0)
    return torch.load(f, weights_only=True)


# ---- 1. the average is the recurrence over the weights the optimiser left ----------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("mode", ["full", "enc-head-ft-dec-head-ft"])
def test_average_is_the_recurrence_over_the_weights_of_every_step(dtype, mode):
    eng = _engine(dtype, mode=mode, weight_ema=DECAY)
    fl = eng.flat
    if mode != "full":
        assert len(fl.ranges) > 1 and sum(b - a for a, b in fl.ranges) < fl.n, "the mode was to leave frozen elements between ranges"
    fl.ema.fill_(float("nan"))                       # memory nobody initialised: the first update stores, a frozen element is never touched
    for a in eng.aux:
        if "ema" in a:
            a["ema"].fill_(float("nan"))
    want, st = {}, (0, 0.0)
    for i in range(1, 7):                            # steps 1 - 2 eager, the third call captures, 4 - 6 replay
        out = _step(eng, i)
        torch.cuda.synchronize()
        for k, (p, _) in _averaged(eng).items():
            want[k] = R.update(_np(p), want.get(k), st[0], DECAY)
        st = R.advance(st, DECAY)
        assert float(out["weight_ema_decay"]) == st[1], i
        for k, (_, ema) in _averaged(eng).items():
            bad = R.same_bits(_np(ema), want[k])
            assert bad.size == 0, (i, k, bad[:8].tolist())
    assert eng._graphs and eng.weight_ema_updates == 6 == st[0]
    assert st[1] == float(np.float32(np.float64(6.0) / np.float64(15.0)))
    inside = torch.zeros(fl.n, dtype=torch.bool, device="cuda")
    for a, b in fl.ranges:
        inside[a:b] = True
    assert torch.isnan(fl.ema[~inside]).all() and not torch.isnan(fl.ema[inside]).any()      # nothing outside the ranges was written
    assert all(not torch.isnan(a["ema"]).any() for a in eng.aux if "ema" in a)


# ---- 2. eager = replay ---------------------------------------------------------------------------------------------------------------
@DTYPES
def test_eager_and_replayed_steps_agree_bit_for_bit(dtype):
    eager, graph = _engine(dtype, use_graph=False, weight_ema=DECAY), _engine(dtype, use_graph=True, weight_ema=DECAY)
    for i in range(1, 7):
        oe, og = _step(eager, i), _step(graph, i)
        assert "weight_ema_decay" in oe and "weight_ema_decay" in og
        _assert_same_losses(oe, og, f"step {i}")
        _assert_bits_equal(_snapshot(eager), _snapshot(graph), f"after step {i}")
    assert not eager._graphs and len(graph._graphs) == 1
    for census in next(iter(graph._graphs.values())).node_census():          # the step's graphs still hold kernel nodes only
        assert census["kernel"] > 0 and census["memset"] == census["memcpy"] == census["other"] == 0, census


# ---- 3. off = nothing ------------------------------------------------------------------------------------------------------------------
def test_option_off_calls_none_of_the_entry_points(monkeypatch):
    from kvq import _ffi
    lib = _ffi.lib()

    def boom(*_a):
        raise AssertionError("a weight-EMA entry point was called with the option off")
    for name in ("kvq_weight_ema_update", "kvq_weight_ema_advance", "kvq_weight_ema_swap"):
        monkeypatch.setattr(lib, name, boom)
    eng = _engine(torch.bfloat16)
    for i in range(1, 5):
        out = _step(eng, i)
        assert "weight_ema_decay" not in out
    eng.eval_step(*_batch(1))
    assert eng._graphs and eng.flat._ema is None and eng._wema_state is None and eng.weight_ema is None and eng.weight_ema_updates == 0
    assert all("ema" not in a for a in eng.aux)
    with pytest.raises(_ffi.KvqError, match="weight_ema"):
        with eng.weight_ema_applied():
            pass


# ---- 4. / 5. the scope -----------------------------------------------------------------------------------------------------------------
@DTYPES
def test_evaluation_inside_the_scope_is_evaluation_of_the_averaged_weights_and_leaving_restores_every_bit(dtype):
    from kvq.engine import TrainEngine
    eng, twin = _engine(dtype, weight_ema=DECAY), _engine(dtype, weight_ema=DECAY)
    for i in range(1, 5):
        _step(eng, i), _step(twin, i)
    eng.model.eval()
    ids, mask = _batch(7)
    live = eng.eval_step(ids, mask)                  # (also leaves the codebook pack current for the snapshot)
    before = _snapshot(eng)
    pack_before = eng._epack.clone()
    former = {k: (p.clone(), e.clone()) for k, (p, e) in _averaged(eng).items()}
    versions = eng._versions()
    with eng.weight_ema_applied() as scope:
        assert scope is eng
        torch.cuda.synchronize()
        for k, (p, e) in _averaged(eng).items():
            assert torch.equal(_raw(p), _raw(former[k][1])), (k, "the parameters are not the former average")
            assert torch.equal(_raw(e), _raw(former[k][0])), (k, "the average's buffer does not hold the former parameters")
        if dtype == torch.bfloat16:
            for a, b in eng.flat.ranges:
                assert torch.equal(_raw(eng.flat.shadow[a:b]), _raw(eng.flat.master[a:b].to(torch.bfloat16))), "the shadow was not refreshed"
        assert eng._versions() == versions           # raw-pointer writes: refresh_if_params_changed stays quiet
        sd = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}
        inside = eng.eval_step(ids, mask)
        logits = eng.forward_logits(ids, mask)["logits"].clone()
    assert not torch.equal(_raw(inside["loss_recon"]), _raw(live["loss_recon"])), "the average scored like the live weights"
    # a second engine on a model that LOADED the state_dict taken inside the scope
    other = _shelgon(dtype, seed=4321).eval()
    other.load_state_dict(sd)
    eng2 = TrainEngine(other, lr=LR)
    _assert_same_losses(inside, eng2.eval_step(ids, mask), "eval_step inside the scope against an engine on the averaged weights")
    assert torch.equal(_raw(logits), _raw(eng2.forward_logits(ids, mask)["logits"]))
    # 5. leaving restored master, shadow, average -- and, once the quantiser runs again, the codebook pack
    _assert_bits_equal(_snapshot(eng), before, "after the scope")
    _assert_same_losses(eng.eval_step(ids, mask), live, "eval_step after the scope")
    assert torch.equal(eng._epack, pack_before)
    eng.model.train()
    for i in range(5, 7):                            # the captured chain is still valid, and the steps are the twin's
        _assert_same_losses(_step(eng, i), _step(twin, i), f"step {i} after the scope")
        _assert_bits_equal(_snapshot(eng), _snapshot(twin), f"after step {i}")
    assert len(eng._graphs) == 1


def test_entering_before_any_update_applies_nothing():
    eng = _engine(torch.bfloat16, weight_ema=DECAY)
    before = _raw(eng.flat.master).clone()
    with eng.weight_ema_applied():
        assert torch.equal(_raw(eng.flat.master), before) and eng.flat._ema is None
        eng.eval_step(*_batch(1))
    assert torch.equal(_raw(eng.flat.master), before) and eng.flat._ema is None and eng.weight_ema_updates == 0


# ---- 6. a skipped step does not move the average ---------------------------------------------------------------------------------------
@DTYPES
def test_a_non_finite_step_leaves_the_average_and_its_state_alone(dtype):
    from kvq import nnops
    eng = _engine(dtype, weight_ema=DECAY, max_grad_norm=1.0)
    for i in range(1, 4):
        _step(eng, i)
    before = _snapshot(eng)
    ids, mask = _batch(104)
    eng.forward_backward(ids, mask, compute_grads=True)
    eng.flat.grad[eng.flat.seg["enc.0.f1.w"][0] + 77] = float("nan")
    assert eng.finish_step() is True
    after = _snapshot(eng)
    assert eng.skipped_steps == 1 and eng.step_count == 4
    for k in before:
        if k.startswith("ema.") or k in ("wema_state", "master", "codebook"):
            assert torch.equal(_raw(before[k]), _raw(after[k])), (k, "moved on a skipped step")
    assert nnops.read_weight_ema_state(eng._wema_state) == (3, float(np.float32(np.float64(3.0) / np.float64(12.0))))
    out = _step(eng, 5)
    assert eng.weight_ema_updates == 4 and float(out["weight_ema_decay"]) == float(np.float32(np.float64(4.0) / np.float64(13.0)))


# ---- 7. once per optimiser step ----------------------------------------------------------------------------------------------------------
@DTYPES
def test_with_accumulation_the_average_moves_once_per_cycle(dtype):
    eng = _engine(dtype, weight_ema=DECAY, grad_accum=2)
    ema_words = None
    for call in range(1, 9):                         # both chains are captured by the end
        out = _step(eng, call)
        assert out["optimizer_step"] == (call % 2 == 0) and ("weight_ema_decay" in out) == (call % 2 == 0)
        assert eng.weight_ema_updates == call // 2, call
        if call >= 2:
            words = torch.cat([_raw(e) for _, e in _averaged(eng).values()]).clone()
            if ema_words is not None:                # a micro-step leaves every word, the cycle's last call moves the average
                assert torch.equal(words, ema_words) == (call % 2 == 1), (call, "the average moves on the last call of a cycle only")
            ema_words = words
    assert len(eng._graphs) == 2


# ---- 8. resume ---------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_resumed_run_continues_the_average_bit_for_bit(dtype):
    a, b = _engine(dtype, weight_ema=DECAY), _engine(dtype, weight_ema=DECAY)
    for i in range(1, 4):
        _step(a, i), _step(b, i)
    at3 = _snapshot(a)
    blob = _through_a_file({"engine": b.state_dict(), "model": b.model.state_dict()})
    _assert_bits_equal(_snapshot(b), at3, "state_dict() wrote nothing")
    st = blob["engine"]
    assert st["fingerprint"]["weight_ema"] == DECAY and "ema" in st["flat"] and st["flat"]["ema"].numel() == a.flat.n
    assert all("ema" in d for d in st["aux"]) and st["structs"]["weight_ema"].tolist()[0] == 3
    c = _engine(dtype, seed=4321, weight_ema=DECAY)
    c.model.load_state_dict(blob["model"])
    c.load_state_dict(st)
    _assert_bits_equal(_snapshot(c), at3, "straight after the load")
    for i in range(4, 7):
        _assert_same_losses(_step(a, i), _step(c, i), f"step {i}")
        _assert_bits_equal(_snapshot(c), _snapshot(a), f"after step {i}")
    assert c.weight_ema_updates == 6
    # a state from before the first update holds no flat.ema, and loads
    fresh = _through_a_file(_engine(dtype, weight_ema=DECAY).state_dict())
    assert "ema" not in fresh["flat"] and fresh["structs"]["weight_ema"].tolist() == [0, 0]
    c.load_state_dict(fresh)
    assert c.weight_ema_updates == 0 and c.step_count == 0


# ---- 9. / 10. the state of an engine without the option, and loading across option settings ---------------------------------------------
def test_state_without_the_option_has_todays_keys_and_crossing_is_refused():
    from kvq._ffi import KvqError
    off, on = _engine(torch.bfloat16), _engine(torch.bfloat16, weight_ema=DECAY)
    for i in range(1, 3):
        _step(off, i), _step(on, i)
    s_off, s_on = off.state_dict(), on.state_dict()
    assert set(s_off) == {"format", "kvq_version", "fingerprint", "flat", "aux", "structs", "host"}
    assert set(s_off["fingerprint"]) == FINGERPRINT_KEYS and set(s_off["flat"]) == {"master", "m", "v"}
    assert set(s_off["structs"]) == {"state"} and [set(d) for d in s_off["aux"]] == [{"p", "m", "v"}]
    assert set(s_off["host"]) == {"step", "accum_pending", "grads_are_mean"}
    assert set(s_on) == set(s_off) and set(s_on["fingerprint"]) == FINGERPRINT_KEYS | {"weight_ema"}
    assert set(s_on["flat"]) == {"master", "m", "v", "ema"} and set(s_on["structs"]) == {"state", "weight_ema"}
    assert [set(d) for d in s_on["aux"]] == [{"p", "m", "v", "ema"}]
    for target, state in ((on, s_off), (off, s_on), (on, dict(s_on, fingerprint=dict(s_on["fingerprint"], weight_ema=0.5)))):
        before = _snapshot(target)
        with pytest.raises(KvqError, match=r"fingerprint\.weight_ema"):
            target.load_state_dict(state)
        _assert_bits_equal(_snapshot(target), before, "a refused load wrote something")
    on.load_state_dict(s_on)                         # its own state loads
    missing = dict(s_on, structs={k: v for k, v in s_on["structs"].items() if k != "weight_ema"})
    with pytest.raises(KvqError, match=r"structs\.weight_ema"):
        on.load_state_dict(missing)


# ---- 11. refusals ------------------------------------------------------------------------------------------------------------------------
def test_what_is_refused():
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    with pytest.raises(KvqError, match="fp8"):       # the swapped weights' fp8 mirror: a piece of work of its own
        TrainEngine(_shelgon(torch.bfloat16), lr=LR, weight_ema=DECAY, fp8_forward=True)
    for bad in (0.0, 1.0, 1.5, True, "0.9"):
        with pytest.raises(KvqError, match="weight_ema"):
            TrainEngine(_shelgon(torch.bfloat16), lr=LR, weight_ema=bad)
    eng = _engine(torch.bfloat16, weight_ema=DECAY)
    for i in range(1, 3):
        _step(eng, i)
    state = eng.state_dict()
    ids, mask = _batch(3)
    before = _snapshot(eng)
    with eng.weight_ema_applied():
        inside = _snapshot(eng)
        for what, call in (("train_step", lambda: eng.train_step(ids, mask)),
                           ("forward_backward", lambda: eng.forward_backward(ids, mask, compute_grads=True)),
                           ("finish_step", eng.finish_step), ("optimizer_step", eng.optimizer_step),
                           ("state_dict", eng.state_dict), ("load_state_dict", lambda: eng.load_state_dict(state)),
                           ("weight_ema_applied", lambda: eng.weight_ema_applied().__enter__())):
            with pytest.raises(KvqError, match="weight_ema_applied"):
                call()
        eng.forward_backward(ids, mask, training=False, compute_grads=False)          # forward-only calls are what the scope is for
        _assert_bits_equal(_snapshot(eng), inside, "a refused call wrote something")
    _assert_bits_equal(_snapshot(eng), before, "after the scope")
    with pytest.raises(RuntimeError, match="boom"):  # an exception inside the scope still swaps back
        with eng.weight_ema_applied():
            raise RuntimeError("boom")
    _assert_bits_equal(_snapshot(eng), before, "after a scope left by an exception")
    _step(eng, 3)                                    # and the engine trains on
    assert eng.weight_ema_updates == 3
