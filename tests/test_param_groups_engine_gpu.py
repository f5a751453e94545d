"""TrainEngine(param_groups=..., decoupled_weight_decay=..., lr_warmup_steps=..., lr_decay=...) on kvq-bert-tiny
Shelgon, B = 16, S = 12: groups that resolve to the defaults leave every bit alone; with real groups every step's master buffer and
moments are the f64 grouped reference applied to the engine's OWN gradients of that step (so the check does not depend on GEMM
numerics), eager equals replay, the step's graphs hold what an option-off engine's hold, out["lr"] is the schedule, and the options
compose with max_grad_norm, grad_accum, weight_ema, data parallelism and the training state.  "bits equal" = the raw words."""
import fnmatch
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

import _adam_groups_ref as G
import _adam_ref as R
from test_engine_multiproc_gpu import _build as _build_dp, _data as _data_dp, _free_port, _identical_across_ranks
from test_weight_ema_engine_gpu import (FINGERPRINT_KEYS, LR, _assert_bits_equal, _assert_same_losses, _batch, _engine, _raw, _shelgon,
                                        _snapshot, _step, _through_a_file)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
WD, W, T = 0.01, 3, 6
NO_DECAY = ["*.b", "*.ln.w", "*.ln2.w", "head.bias"]                    # spelled out: the preset itself is compared with it below
GROUPS = [{"match": NO_DECAY, "weight_decay": 0.0}, {"match": "vq.codebook", "lr_scale": 10}, {"match": "enc.*", "lr_scale": 0.1}]
ON = dict(param_groups=GROUPS, weight_decay=WD, lr_warmup_steps=W, lr_decay="cosine", lr_total_steps=T)


@pytest.fixture(autouse=True)
def _no_environment_switch(monkeypatch):
    for name in ("KVQ_WEIGHT_EMA", "KVQ_GRAD_ACCUM", "KVQ_MAX_GRAD_NORM", "KVQ_VQ_REVIVE_AFTER", "KVQ_DP_SINGLE_RANK", "KVQ_FP8",
                 "KVQ_FP8_BACKWARD", "KVQ_GRAPH", "KVQ_PARAM_GROUPS", "KVQ_DECOUPLED_WD", "KVQ_LR_WARMUP_STEPS", "KVQ_LR_DECAY",
                 "KVQ_LR_TOTAL_STEPS", "KVQ_LR_MIN_RATIO"):
        monkeypatch.delenv(name, raising=False)


def expected_rule(name):
    """(lr scale, weight decay) of a parameter under GROUPS, restated without the engine's resolver: first match wins."""
    if any(fnmatch.fnmatchcase(name, p) for p in NO_DECAY):
        return 1.0, 0.0
    if name == "vq.codebook":
        return 10.0, WD
    if name.startswith("enc."):
        return 0.1, WD
    return 1.0, WD


def _pre(eng):
    torch.cuda.synchronize()
    fl = eng.flat
    return dict(p=fl.master.clone(), m=fl.m.clone(), v=fl.v.clone(), aux=[{k: a[k].clone() if k != "p" else a["p"].data.clone()
                                                                           for k in ("p", "m", "v")} for a in eng.aux])


def _judge_step(eng, pre, lr, t, decoupled):
    """Worst ratio per judged output of one applied step: the flat buffer's trainable parameter elements and the aux parameters
    against G.grouped_ref of the pre-state and the engine's own gradients, under the judges' counted bounds."""
    torch.cuda.synchronize()
    fl, grads = eng.flat, eng.grads_by_parameter()
    hp = R.hyper(lr, eng.betas[0], eng.betas[1], eng.eps, 0.0, 1.0, t)
    g = torch.zeros(fl.n, dtype=torch.float32, device="cuda")
    mask = torch.zeros(fl.n, dtype=torch.bool, device="cuda")
    s_e, wd_e = torch.ones(fl.n, dtype=torch.float64, device="cuda"), torch.zeros(fl.n, dtype=torch.float64, device="cuda")
    for name, p in eng.param_of.items():
        o, n, _ = fl.seg[name]
        s_e[o:o + n], wd_e[o:o + n] = R.f32(expected_rule(name)[0]), R.f32(expected_rule(name)[1])
        if p.requires_grad:
            g[o:o + n] = grads[p].reshape(-1).float()
            mask[o:o + n] = True
    x = dict(p=pre["p"], m=pre["m"], v=pre["v"], g=g, vmax=None)
    ratios = G.grouped_ratios(dict(p=fl.master, m=fl.m, v=fl.v, vmax=None), x, hp, s_e, wd_e, decoupled)
    worst = {k: float(r[mask].max()) for k, r in ratios.items()}
    for a, b in zip(eng.aux, pre["aux"]):
        n = a["p"].numel()
        sc, wd = expected_rule(a["name"])
        xa = dict(p=b["p"].view(-1), m=b["m"].view(-1), v=b["v"].view(-1), g=grads[a["p"]].reshape(-1).float(), vmax=None)
        ra = G.grouped_ratios(dict(p=a["p"].data.view(-1), m=a["m"].view(-1), v=a["v"].view(-1), vmax=None), xa, hp,
                              torch.full((n,), R.f32(sc), dtype=torch.float64, device="cuda"),
                              torch.full((n,), R.f32(wd), dtype=torch.float64, device="cuda"), decoupled)
        worst.update({f"{a['name']}.{k}": float(r.max()) for k, r in ra.items()})
    return worst, int(mask.sum())


def _census(eng):
    assert len(eng._graphs) == 1
    return next(iter(eng._graphs.values())).node_census()


# ---- 1. default-only groups change no bit --------------------------------------------------------------------------------------------
@DTYPES
def test_groups_that_resolve_to_the_defaults_leave_every_bit(dtype):
    off = _engine(dtype, weight_decay=WD)
    on = _engine(dtype, weight_decay=WD, param_groups=[{"match": "*"}, {"match": ["enc.0.*"], "lr_scale": 1.0, "weight_decay": WD}])
    assert on._pg is not None and on.param_group_of("enc.0.f1.w") == 1 and on.decoupled_wd is False and on.lr_schedule is None
    for i in range(1, 5):                            # steps 1 - 2 eager, the third call captures, the fourth replays
        oa, ob = _step(off, i), _step(on, i)
        _assert_same_losses(oa, ob, f"step {i}")
        assert "lr" not in ob
        _assert_bits_equal(_snapshot(off), _snapshot(on), f"after step {i}")
    assert _census(on) == _census(off)


# ---- 2. every step is the reference applied to the engine's own gradients ------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("decoupled", [False, True], ids=["coupled", "decoupled"])
def test_every_step_is_the_grouped_reference_on_the_engines_own_gradients(dtype, decoupled):
    from kvq.engine import NO_DECAY as PRESET
    assert PRESET == NO_DECAY
    eng = _engine(dtype, decoupled_weight_decay=decoupled, **ON)
    for name in eng.param_names():                   # the engine's resolution is the restated rule
        g = eng.param_group_table()[eng.param_group_of(name)]
        assert (g["lr_scale"], g["weight_decay"]) == expected_rule(name), name
    table = eng.param_group_table()
    assert [g["group"] for g in table] == [0, 1, 2, 3] and table[2]["names"] == 1 and table[2]["elements"] == eng.E.numel()
    assert sum(g["names"] for g in table) == len(eng.param_names()) and all(g["elements"] > 0 for g in table)
    worst_all = {}
    for t in range(1, 7):
        pre = _pre(eng)
        out = _step(eng, t)
        lr = float(out["lr"])
        ref = G.sched_ref(t, LR, 0.1, [], W, 2, T, 0.0)
        assert G.sched_ratio(lr, ref, LR) <= 1.0, (t, lr, ref)
        assert abs(eng._lr_now() - ref) <= 2.0 ** -23 * ref + 1e-20, (t, eng._lr_now(), ref)      # the host mirror starts from the unrounded lr
        worst, judged = _judge_step(eng, pre, lr, t, decoupled)
        assert judged > 100000
        print(f"FIGURE step {t} lr {lr:.6e}: " + ", ".join(f"{k} {w:.4f}" for k, w in sorted(worst.items())))
        assert max(worst.values()) <= 1.0, (t, worst)
        for k, w in worst.items():
            worst_all[k] = max(w, worst_all.get(k, 0.0))
    assert eng._graphs and eng.step_count == 6 and float(out["lr"]) <= G.SCHED_ABS * LR          # cosine to min_ratio 0 at T = 6
    assert set(worst_all) == {"m", "v", "p", "vq.codebook.m", "vq.codebook.v", "vq.codebook.p"}


# ---- 3. eager = replay, and the graphs hold what an option-off engine's hold -------------------------------------------------------------
@DTYPES
def test_eager_equals_replay_and_the_graph_census_is_the_option_off_engines(dtype):
    eager = _engine(dtype, use_graph=False, decoupled_weight_decay=True, **ON)
    graph = _engine(dtype, use_graph=True, decoupled_weight_decay=True, **ON)
    off = _engine(dtype, weight_decay=WD)
    for i in range(1, 7):
        oe, og = _step(eager, i), _step(graph, i)
        _step(off, i)
        _assert_same_losses(oe, og, f"step {i}")
        assert torch.equal(_raw(oe["lr"]), _raw(og["lr"])), i
        _assert_bits_equal(_snapshot(eager), _snapshot(graph), f"after step {i}")
    assert not eager._graphs
    census = _census(graph)
    assert census == _census(off), (census, _census(off))
    for c in census:
        assert c["kernel"] > 0 and c["memset"] == c["memcpy"] == c["other"] == 0, c
    moved = _snapshot(graph)
    assert not torch.equal(moved["master"], _snapshot(off)["master"])


# ---- 4. composition ---------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_a_non_finite_gradient_leaves_every_groups_state_untouched(dtype):
    eng = _engine(dtype, decoupled_weight_decay=True, max_grad_norm=1.0, **ON)
    for i in range(1, 4):
        out = _step(eng, i)
        assert "grad_norm" in out and "lr" in out
    before = _snapshot(eng)
    ids, mask = _batch(104)
    eng.forward_backward(ids, mask, compute_grads=True)
    eng.flat.grad[eng.flat.seg["enc.0.f1.w"][0] + 77] = float("nan")
    assert eng.finish_step() is True
    after = _snapshot(eng)
    assert eng.skipped_steps == 1 and eng.step_count == 4
    for k in before:                                 # the step state moves on (the schedule too), nothing Adam owns does
        if k not in ("state", "guard"):
            assert torch.equal(_raw(before[k]), _raw(after[k])), (k, "moved on a skipped step")
    pre = _pre(eng)                                  # and the next step is a clipped, grouped step under the judges
    out = _step(eng, 5)
    hp_lr = float(out["lr"])
    assert G.sched_ratio(hp_lr, G.sched_ref(5, LR, 0.1, [], W, 2, T, 0.0), LR) <= 1.0
    assert not torch.equal(_raw(pre["p"]), _raw(eng.flat.master))


@DTYPES
def test_with_accumulation_the_grouped_update_runs_once_per_cycle_on_the_mean(dtype):
    eng = _engine(dtype, decoupled_weight_decay=False, grad_accum=2, **ON)
    for call in range(1, 9):
        pre = _pre(eng)
        out = _step(eng, call)
        torch.cuda.synchronize()
        assert out["optimizer_step"] == (call % 2 == 0) and ("lr" in out) == (call % 2 == 0)
        if call % 2:
            assert torch.equal(_raw(pre["p"]), _raw(eng.flat.master)) and torch.equal(_raw(pre["m"]), _raw(eng.flat.m)), call
        else:                                        # grads_by_parameter() is then the cycle's mean: what Adam read, as f32
            t = call // 2
            worst, _ = _judge_step(eng, pre, float(out["lr"]), t, False)
            assert max(worst.values()) <= 1.0, (call, worst)
    assert len(eng._graphs) == 2 and eng.step_count == 4


@DTYPES
def test_the_weight_average_follows_the_grouped_weights(dtype):
    import numpy as np
    import _weight_ema_ref as WR
    from test_weight_ema_engine_gpu import _averaged, _np
    eng = _engine(dtype, decoupled_weight_decay=True, weight_ema=0.999, **ON)
    want, st = {}, (0, 0.0)
    for i in range(1, 5):
        _step(eng, i)
        torch.cuda.synchronize()
        for k, (p, _) in _averaged(eng).items():
            want[k] = WR.update(_np(p), want.get(k), st[0], 0.999)
        st = WR.advance(st, 0.999)
        for k, (_, ema) in _averaged(eng).items():
            assert WR.same_bits(_np(ema), want[k]).size == 0, (i, k)
    assert eng.weight_ema_updates == 4


def _worker_dp(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))
    import torch.distributed as dist
    from kvq import ddp
    from kvq.engine import TrainEngine
    torch.cuda.set_device(0)
    ddp.init_distributed("gloo")
    ids, mask = _data_dp()
    half = slice(rank * 4, rank * 4 + 4)
    report = {}
    for tag, use_graph in (("eager", False), ("graph", True)):
        model = _build_dp()
        ddp.broadcast_parameters(model)
        eng = TrainEngine(model, lr=1e-3, bucket_mib=0, decoupled_weight_decay=True, **ON)      # many small chunks: clipped Adam ranges
        eng.use_graph = use_graph
        assert eng.world == 2 and eng._dp and eng._pg is not None
        start = eng.flat.master.clone()
        for step in range(1, 5):
            eng.train_step(ids[half], mask[half])
            torch.cuda.synchronize()
            report[(tag, step)] = {k: _identical_across_ranks(t) for k, t in
                                   dict(master=eng.flat.master, m=eng.flat.m, v=eng.flat.v, codebook=eng.E.data, state=eng._state.view(torch.int32)).items()}
        report[tag + "_moved"] = float((eng.flat.master - start).abs().max())
        report[tag + "_first_elements"] = sorted(a for (a, b) in eng._pg["range_group"])
        del eng, model
    if rank == 0:
        torch.save(report, out)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_stay_bit_identical_under_groups(tmp_path):
    out = str(tmp_path / "dp_groups.pt")
    mp.spawn(_worker_dp, args=(2, _free_port(), out), nprocs=2, join=True)
    rep = torch.load(out)
    for tag in ("eager", "graph"):
        assert rep[tag + "_moved"] > 1e-5
        assert any(a > 0 for a in rep[tag + "_first_elements"]), "no Adam launch started inside the buffer: the cut was not exercised"
        for step in range(1, 5):
            bad = [k for k, ok in rep[(tag, step)].items() if not ok]
            assert not bad, f"{tag} step {step}: ranks differ in {bad}"


# ---- 5. training state ---------------------------------------------------------------------------------------------------------------------
def test_training_state_keys_crossing_and_resume():
    from kvq._ffi import KvqError
    off = _engine(torch.bfloat16, weight_decay=WD)
    a, b = (_engine(torch.bfloat16, decoupled_weight_decay=True, **ON) for _ in range(2))
    for i in range(1, 4):
        _step(off, i), _step(a, i), _step(b, i)
    s_off, s_on = off.state_dict(), b.state_dict()
    assert set(s_off["fingerprint"]) == FINGERPRINT_KEYS and set(s_off["structs"]) == {"state"} and set(s_off["flat"]) == {"master", "m", "v"}
    assert set(s_on["fingerprint"]) == FINGERPRINT_KEYS | {"param_groups", "decoupled_weight_decay", "lr_schedule"}
    assert set(s_on["structs"]) == {"state"} and set(s_on["flat"]) == {"master", "m", "v"}          # no new tensor is state
    assert s_on["fingerprint"]["lr_schedule"] == [W, "cosine", T, 0.0] and s_on["fingerprint"]["decoupled_weight_decay"] is True
    assert [g[:3] for g in s_on["fingerprint"]["param_groups"]][1:] == [[NO_DECAY, 1.0, 0.0], [["vq.codebook"], 10.0, WD], [["enc.*"], 0.1, WD]]
    only = lambda **kw: _engine(torch.bfloat16, weight_decay=WD, **kw)
    assert set(only(lr_warmup_steps=2).state_fingerprint()) == FINGERPRINT_KEYS | {"lr_schedule"}
    assert set(only(decoupled_weight_decay=True).state_fingerprint()) == FINGERPRINT_KEYS | {"decoupled_weight_decay"}
    assert set(only(param_groups=GROUPS).state_fingerprint()) == FINGERPRINT_KEYS | {"param_groups"}
    fp = s_on["fingerprint"]
    other = [list(g) for g in fp["param_groups"]]
    other[2] = [other[2][0], 5.0] + other[2][2:]
    for target, state, key in ((b, s_off, "param_groups"), (off, s_on, "param_groups"), (off, s_on, "lr_schedule"),
                               (off, s_on, "decoupled_weight_decay"),
                               (b, dict(s_on, fingerprint=dict(fp, param_groups=other)), "param_groups"),
                               (b, dict(s_on, fingerprint=dict(fp, lr_schedule=[W, "linear", T, 0.0])), "lr_schedule"),
                               (b, dict(s_on, fingerprint={k: v for k, v in fp.items() if k != "decoupled_weight_decay"}), "decoupled_weight_decay")):
        before = _snapshot(target)
        with pytest.raises(KvqError, match=rf"fingerprint\.{key}"):
            target.load_state_dict(state)
        _assert_bits_equal(_snapshot(target), before, "a refused load wrote something")
    at3 = _snapshot(a)
    blob = _through_a_file({"engine": s_on, "model": b.model.state_dict()})
    c = _engine(torch.bfloat16, seed=4321, decoupled_weight_decay=True, **ON)
    c.model.load_state_dict(blob["model"])
    c.load_state_dict(blob["engine"])
    _assert_bits_equal(_snapshot(c), at3, "straight after the load")
    for i in range(4, 7):
        oa, oc = _step(a, i), _step(c, i)
        _assert_same_losses(oa, oc, f"step {i}")
        assert torch.equal(_raw(oa["lr"]), _raw(oc["lr"]))
        _assert_bits_equal(_snapshot(c), _snapshot(a), f"after step {i}")


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_what_is_refused():
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    with pytest.raises(KvqError, match="fp8"):
        TrainEngine(_shelgon(torch.bfloat16), lr=LR, param_groups=GROUPS, fp8_forward=True)
    with pytest.raises(KvqError, match="fp8"):
        TrainEngine(_shelgon(torch.bfloat16), lr=LR, decoupled_weight_decay=True, fp8_forward=True)
    model = _shelgon(torch.bfloat16)
    word = model.encoder.embeddings.word_embeddings.weight
    ptr = word.data_ptr()
    with pytest.raises(KvqError, match=r"enc\.\*\.nonsense"):
        TrainEngine(model, lr=LR, param_groups=[{"match": ["enc.*.nonsense"]}])
    assert word.data_ptr() == ptr and "_kvq_engine" not in model.__dict__, "a refused constructor laid something out"
    with pytest.raises(KvqError, match="16 groups"):
        TrainEngine(model, lr=LR, param_groups=[{"match": "enc.*"}] * 16)
    with pytest.raises(KvqError, match="lr_total_steps"):
        TrainEngine(model, lr=LR, lr_decay="cosine", lr_warmup_steps=3, lr_total_steps=3)
    eng = TrainEngine(_shelgon(torch.bfloat16), lr=LR, fp8_forward=True, lr_warmup_steps=2)     # the schedule alone composes with fp8
    out = [eng.train_step(*_batch(100 + i)) for i in range(1, 4)]
    assert [float(o["lr"]) for o in out] == [R.f32(R.f32(LR) * 0.5), R.f32(LR), R.f32(LR)]
    assert "vq.codebook" in eng.param_names() and eng.param_group_of("vq.codebook") == 0 and len(eng.param_group_table()) == 1
