"""Host side of free-running generation, no GPU: kvq.functional.shift_right, the DECODER_NEXT_TOKEN plumbing of both trainers
(a stub engine records what it is handed), the ctypes table of the kvq_gen_* entry points against include/kvq.h, and the
argument checks of TrainEngine.generate that need no device."""
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")


def test_shift_right_on_ragged_padded_batches():
    from kvq._ffi import KvqError
    from kvq.functional import shift_right
    ids = torch.tensor([[11, 12, 13, 14, 15], [21, 22, 0, 0, 0], [31, 0, 0, 0, 0], [0, 0, 0, 0, 0]])
    mask = (ids != 0).long()
    keep = ids.clone()
    got = shift_right(ids, 101)
    assert got.tolist() == [[101, 11, 12, 13, 14], [101, 21, 22, 0, 0], [101, 31, 0, 0, 0], [101, 0, 0, 0, 0]]
    assert shift_right(mask, 1).tolist() == [[1, 1, 1, 1, 1], [1, 1, 1, 0, 0], [1, 1, 0, 0, 0], [1, 0, 0, 0, 0]]
    assert torch.equal(ids, keep) and got.dtype == ids.dtype and got.data_ptr() != ids.data_ptr()
    # position t of the shifted row holds only tokens before t: the target ids[t] is not among the decoder's input up to t
    for t in range(5):
        assert torch.equal(got[:, 1:t + 1], ids[:, :t])
    assert shift_right(torch.tensor([[7]]), 3).tolist() == [[3]]
    assert shift_right(torch.arange(24).view(2, 3, 4), 9)[1, 2].tolist() == [9, 20, 21, 22]
    for bad in (lambda: shift_right([1, 2], 0), lambda: shift_right(torch.zeros(2, 0, dtype=torch.int64), 0), lambda: shift_right(ids, 1.5),
                lambda: shift_right(ids, True)):
        with pytest.raises(KvqError):
            bad()


class StubEngine:
    def __init__(self):
        self.calls = []

    def _out(self, ids):
        z = torch.zeros(())
        return dict(loss_recon=z, loss_vq=z, perplexity=z, acc=z, acc_per_sentence=torch.zeros(ids.shape[0]), recon_ids=ids)

    def train_step(self, ids, mask, **kw):
        self.calls.append(("train", ids, mask, kw))
        return self._out(ids)

    def eval_step(self, ids, mask, **kw):
        self.calls.append(("eval", ids, mask, kw))
        return self._out(ids)


IDS = torch.tensor([[101, 1005, 1006, 102, 0, 0], [101, 1007, 102, 0, 0, 0]])
MASK = (IDS != 0).long()


def _shelgon_step(model, engine, opt):
    from models.shelgon3.Trainer import step
    return step("cpu", model, None, True, opt, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, None, dict(input_ids=IDS, attention_mask=MASK, packed="PACK"),
                2048, "train", engine=engine)


def _bagon_step(model, engine, opt):
    from models.bagon.Trainer import step
    return step("cpu", model, None, None, True, 6, True, 6, 0.0, 0.0, opt, None, dict(input_ids=IDS, attention_mask=MASK, packed="PACK"),
                2048, 2048, engine=engine)


@pytest.mark.parametrize("run", [_shelgon_step, _bagon_step])
def test_next_token_option_shifts_the_decoder_input_and_scores_against_the_ids(run):
    eng = StubEngine()
    on = SimpleNamespace(decoder_next_token_start_id=101)
    for opt, name in ((object(), "train"), (None, "eval")):
        run(on, eng, opt)
        kind, ids, mask, kw = eng.calls[-1]
        assert kind == name and torch.equal(ids, IDS) and torch.equal(mask, MASK)
        assert {k for k, v in kw.items() if v is not None} == {"dec_ids", "dec_mask", "target_ids"}      # (no packed batch: it carries the encoder's sort only)
        assert kw["dec_ids"].tolist() == [[101, 101, 1005, 1006, 102, 0], [101, 101, 1007, 102, 0, 0]]
        assert kw["dec_mask"].tolist() == [[1, 1, 1, 1, 1, 0], [1, 1, 1, 1, 0, 0]]
        assert kw["target_ids"] is ids or torch.equal(kw["target_ids"], IDS)
    # off (the default): the step hands the engine exactly what it handed it before the option existed
    off = SimpleNamespace()
    run(off, eng, object())
    kind, ids, mask, kw = eng.calls[-1]
    assert kind == "train" and kw == {"prepared": "PACK"} and torch.equal(ids, IDS)
    run(off, eng, None)
    assert eng.calls[-1][0] == "eval" and eng.calls[-1][3] == {}
    # the autograd path has no target of its own: the option is refused there, not ignored
    with pytest.raises(ValueError, match="DECODER_NEXT_TOKEN"):
        run(on, None, None)


def test_both_configurations_carry_the_option_off_by_default():
    import importlib
    for sub in ("shelgon3", "bagon"):
        sys.path.insert(0, os.path.join(PKG, "models", sub))
        try:
            sys.modules.pop("config", None)
            cfg = importlib.import_module("config")
            assert cfg.DECODER_NEXT_TOKEN is False and cfg.get_config()["decoder_next_token"] is False
            os.environ["KVQ_DECODER_NEXT_TOKEN"] = "True"
            assert importlib.reload(cfg).DECODER_NEXT_TOKEN is True
            os.environ["KVQ_DECODER_NEXT_TOKEN"] = "1"                             # the environment's 0 / 1, as KVQ_LOSS_IGNORE_PAD
            assert importlib.reload(cfg).DECODER_NEXT_TOKEN is True
            os.environ["KVQ_DECODER_NEXT_TOKEN"] = "0"
            assert importlib.reload(cfg).DECODER_NEXT_TOKEN is False
            os.environ["KVQ_DECODER_NEXT_TOKEN"] = "2"
            with pytest.raises(ValueError, match="DECODER_NEXT_TOKEN"):
                importlib.reload(cfg)
        finally:
            os.environ.pop("KVQ_DECODER_NEXT_TOKEN", None)
            sys.path.pop(0)
            sys.modules.pop("config", None)


def test_ffi_table_binds_the_generation_entry_points_with_the_headers_arity():
    from kvq import _ffi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kvq.h")).read(), flags=re.S)
    names = ("kvq_gen_embed", "kvq_gen_attn", "kvq_gen_select", "kvq_gen_advance", "kvq_gen_gumbel_debug")
    for name in names:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/kvq.h"
        params = [p.strip() for p in m.group(1).split(",")]
        res, args = _ffi.SIGNATURES[name]
        assert res is _ffi._int and len(args) == len(params), name
        for p, a in zip(params, args):                                            # pointers as void*, 64-bit integers as such
            want = _ffi._vp if "*" in p else (_ffi._i64 if p.startswith("int64_t") else (_ffi.C.c_uint64 if p.startswith("uint64_t") else
                                             (_ffi._f32 if p.startswith("float") else _ffi._int)))
            assert a is want, (name, p)
    lib = _ffi.lib()
    assert lib.kvq_version() == 100
    for name in names:                                                            # null arguments are refused before any HIP call
        args = [None if a is _ffi._vp else 0 for a in _ffi.SIGNATURES[name][1]]
        assert getattr(lib, name)(*args) == -1 and lib.kvq_last_error()


def test_generate_refuses_bad_arguments_without_a_device():
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    dev = torch.device("cpu")
    lat = torch.zeros(6, 12, 128)
    prompt = torch.full((6, 1), 101, dtype=torch.int64)
    check = lambda la=lat, L=20, p=prompt, tau=0.0, dt=torch.float32, **kw: TrainEngine._check_generate(la, L, p, 128, dt, dev, 64, tau, V=2048, **kw)
    check()
    check(eos_id=102, pad_id=0, seed=(1 << 64) - 1, tau=0.7)
    for kw, text in ((dict(la=torch.zeros(6, 12, 64)), "latents must be"), (dict(la=torch.zeros(6, 12)), "latents must be"), (dict(la="x"), "latents must be"),
                     (dict(dt=torch.bfloat16), "contiguous"), (dict(la=torch.zeros(6, 24, 128)[:, ::2]), "contiguous"),
                     (dict(la=torch.zeros(0, 12, 128), p=prompt[:0]), "empty"),
                     (dict(L=0), "positive int"), (dict(L=20.0), "positive int"), (dict(L=True), "positive int"), (dict(L=65), "position table"),
                     (dict(p=prompt[:5]), "prompt_ids must be"), (dict(p=prompt.int()), "prompt_ids must be"), (dict(p=prompt.view(-1)), "prompt_ids must be"),
                     (dict(p=torch.zeros(6, 0, dtype=torch.int64)), "prompt_ids must be"), (dict(p=None), "prompt_ids must be"),
                     (dict(L=3, p=torch.zeros(6, 4, dtype=torch.int64)), "does not fit"),
                     (dict(eos_id=True), "eos_id"), (dict(eos_id=2048), "eos_id"), (dict(eos_id=-1), "eos_id"), (dict(eos_id=3.0), "eos_id"),
                     (dict(pad_id=2048), "pad_id"), (dict(pad_id=False), "pad_id"), (dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed"),
                     (dict(seed=0.5), "seed"), (dict(seed=True), "seed"),
                     (dict(p=torch.full((6, 1), 2048, dtype=torch.int64)), "outside"), (dict(p=torch.full((6, 2), -1, dtype=torch.int64)), "outside"),
                     (dict(tau=-0.5), "temperature"), (dict(tau=float("nan")), "temperature"), (dict(tau=float("inf")), "temperature")):
        with pytest.raises(KvqError, match=text):
            check(**kw)
    f32, bf16 = SimpleNamespace(dtype=torch.float32), SimpleNamespace(dtype=torch.bfloat16)
    TrainEngine._seq_limit(f32, "generate", 12, 32)
    TrainEngine._seq_limit(bf16, "generate", 128, 128)
    for eng, lens in ((f32, (12, 33)), (f32, (33, 20)), (bf16, (12, 129))):
        with pytest.raises(KvqError, match="TrainEngine.generate: sequence length"):
            TrainEngine._seq_limit(eng, "generate", *lens)
    from kvq import nnops
    assert nnops.gen_state_words(3, 2, 20, None, 0) == [3, 2, 20, -1, 0, 0, 0, 0] and nnops.gen_state_words(0, 1, 8, 102, 7)[3:5] == [102, 7]
    # temperature and seed: the f32 bits of 1 / temperature and the two halves of the 64-bit key, as int32 words
    assert nnops.gen_state_words(0, 1, 8, None, 0, 0.5, (1 << 63) + 5)[5:] == [5, -(1 << 31), 0x40000000]
    assert nnops.gen_state_words(0, 1, 8, None, 0, 0.0, 77)[5:] == [77, 0, 0]
    for bad in (dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=1e-45), dict(seed=-1), dict(seed=1 << 64), dict(seed=2.0)):
        with pytest.raises(KvqError):
            nnops.gen_state_words(0, 1, 8, None, 0, **bad)
    with pytest.raises(KvqError):
        nnops.gen_advance(torch.zeros(8, dtype=torch.int32))                       # a CPU tensor: there is no CPU path
    with pytest.raises(KvqError):
        nnops.gen_advance(torch.zeros(4, dtype=torch.int64))
