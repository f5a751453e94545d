"""Host-side checks of the loss over real tokens (TrainEngine(loss_ignore_pad=True)): the f64 reference the
GPU tests judge by against F.cross_entropy(ignore_index=...) and its autograd gradient, the option's validation (no device needed),
both entry-point configurations, the header and the ctypes table."""
import importlib
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F

import _ce_ignore_ref as RI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")
ENTRY_POINTS = ("kvq_ce_forward_ignore", "kvq_ce_forward_stats_ignore", "kvq_ce_backward_ignore", "kvq_ce_backward_bias_ignore",
                "kvq_seq_acc_ignore")


def _config(model):
    sys.path.insert(0, os.path.join(PKG, "models", model))
    try:
        sys.modules.pop("config", None)
        return importlib.import_module("config")
    finally:
        sys.path.pop(0)
        sys.modules.pop("config", None)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["zero", "last", "minus100"])
@pytest.mark.parametrize("V", [1, 5, 1027])
def test_reference_equals_torch_cross_entropy_with_ignore_index(which, V):
    N, g_loss = 37, 1.7
    ign = {"zero": 0, "last": V - 1, "minus100": -100}[which]
    g = torch.Generator().manual_seed(V + 3)
    x = (2 * torch.randn(N, V, generator=g)).double()
    t = torch.randint(0, V, (N,), generator=g)
    t[::3] = ign                                                          # ignored rows (with ign inside [0, V): some more by chance)
    if V == 1 and ign == 0:
        t[:] = 0                                                          # every row ignored: handled below
    t[1] = V - 1 if ign != V - 1 or V == 1 else 0
    counted = t != ign
    if V == 1 and ign in (0, V - 1):
        assert int(counted.sum()) == 0
    ref = RI.ce_ignore_ref(x, t, ign, g_loss)
    assert ref["count"] == int(counted.sum()) and torch.equal(ref["counted"], counted)
    if ref["count"] == 0:                                                 # torch: NaN; here: zeros (the documented deviation)
        assert ref["loss"] == 0.0 and ref["acc"] == 0.0 and not ref["grad"].any() and not ref["row_loss"].any()
        assert torch.isnan(F.cross_entropy(x, t, ignore_index=ign, reduction="mean"))
        return
    xg = x.clone().requires_grad_(True)
    loss = F.cross_entropy(xg, t, ignore_index=ign, reduction="mean")
    (loss * g_loss).backward()
    assert abs(ref["loss"] - float(loss.detach())) <= 1e-12
    assert float((ref["grad"] - xg.grad).abs().max()) <= 1e-12
    assert not ref["grad"][~counted].any() and not ref["row_loss"][~counted].any() and not ref["lse"][~counted].any()
    assert torch.all(ref["pred"][~counted] == ign)
    am = x.argmax(dim=1)
    assert torch.equal(ref["pred"][counted], am[counted])
    assert ref["acc"] == float((am[counted] == t[counted]).double().mean())


def test_reference_never_looks_at_an_ignored_row():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(9, 13, generator=g).double()
    t = torch.randint(0, 13, (9,), generator=g)
    t[[0, 4, 8]] = -100
    a = RI.ce_ignore_ref(x, t, -100, 1.7)
    x[[0, 4, 8]] = float("nan")
    b = RI.ce_ignore_ref(x, t, -100, 1.7)
    for k in ("lse", "row_loss", "pred", "grad", "cp", "absmax"):
        assert torch.equal(a[k], b[k]) and torch.all(torch.isfinite(b[k].double())), k
    assert a["loss"] == b["loss"] and a["acc"] == b["acc"] and b["count"] == 6


def test_sentence_accuracy_reference():
    t = torch.tensor([[5, 6, 0, 0], [0, 0, 0, 0], [1, 2, 3, 4]])
    p = torch.tensor([[5, 9, 0, 0], [0, 0, 0, 0], [1, 2, 3, 0]])
    assert RI.seq_acc_ignore_ref(p, t, 0).tolist() == [0.5, 0.0, 0.75]
    assert RI.seq_acc_ignore_ref(p, t, -100).tolist() == [0.75, 1.0, 0.75]


# ---- the option --------------------------------------------------------------------------------------------------------------------
def test_option_validation_needs_no_device(monkeypatch):
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    monkeypatch.delenv("KVQ_LOSS_IGNORE_PAD", raising=False)
    check = TrainEngine.check_loss_ignore_pad
    assert check(None) is False and check(None, env=True) is False             # unset: off
    assert check(True) is True and check(False) is False and check(True, env=True) is True
    monkeypatch.setenv("KVQ_LOSS_IGNORE_PAD", "")
    assert check(None, env=True) is False                                      # empty: off
    monkeypatch.setenv("KVQ_LOSS_IGNORE_PAD", "0")
    assert check(None, env=True) is False
    monkeypatch.setenv("KVQ_LOSS_IGNORE_PAD", "1")
    assert check(None, env=True) is True and check(None) is False and check(False, env=True) is False     # an argument wins
    for bad in (0, 1, 1.0, "1", "True", [True], -100):
        with pytest.raises(KvqError, match="loss_ignore_pad"):
            check(bad)
    for bad in ("2", "-1", "x", "True", "yes"):
        monkeypatch.setenv("KVQ_LOSS_IGNORE_PAD", bad)
        with pytest.raises(KvqError, match="loss_ignore_pad"):
            check(None, env=True)


@pytest.mark.parametrize("model", ["shelgon3", "bagon"])
def test_config_carries_the_switch_and_honours_the_environment(model, monkeypatch):
    monkeypatch.delenv("KVQ_LOSS_IGNORE_PAD", raising=False)
    cfg = _config(model)
    assert cfg.LOSS_IGNORE_PAD is False and cfg.get_config()["loss_ignore_pad"] is False
    for text, want in (("1", True), ("0", False), ("True", True), ("False", False), ("", False), (" ", False)):
        monkeypatch.setenv("KVQ_LOSS_IGNORE_PAD", text)                        # the environment wins; empty: unset
        got = _config(model).LOSS_IGNORE_PAD
        assert got is want, (text, got)
    for bad in ("2", "-1", "0.5", "x", "None", "'yes'", "[True]"):
        monkeypatch.setenv("KVQ_LOSS_IGNORE_PAD", bad)
        with pytest.raises(ValueError, match="LOSS_IGNORE_PAD"):
            _config(model)
    monkeypatch.delenv("KVQ_LOSS_IGNORE_PAD")
    main = open(os.path.join(PKG, "models", model, "main.py")).read()
    assert "loss_ignore_pad=LOSS_IGNORE_PAD" in main and '"loss_ignore_pad"' in main
    trainer = open(os.path.join(PKG, "models", model, "Trainer.py")).read()
    assert "ignore_index=" in trainer and "weighted by" in trainer


def test_header_declares_the_entry_points_and_the_ctypes_table_knows_them():
    from kvq import _ffi
    hdr = open(os.path.join(ROOT, "include", "kvq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _ffi.lib()
    for name in ENTRY_POINTS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", code)
        assert m and "int64_t ignore_index" in m.group(1), name
        assert len(m.group(1).split(",")) == len(_ffi.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert [len(_ffi.SIGNATURES[n][1]) for n in ENTRY_POINTS] == [14, 15, 12, 14, 7]
    assert lib.kvq_version() == 100
    assert "DEVIATES FROM TORCH" in hdr


def test_entry_points_refuse_before_any_launch():
    """N > 2^24 (the f32 count would not be exact) and a missing count pointer are refused by the argument checks, before any HIP call."""
    from kvq import _ffi
    lib = _ffi.lib()
    one = 16          # any non-null address: the checks come first, nothing is dereferenced
    big = (1 << 24) + 1
    assert lib.kvq_ce_forward_ignore(one, one, big, 8, 8, 0, 0, one, one, one, None, None, None, None) != 0
    assert b"kvq_ce_forward_ignore" in lib.kvq_last_error()
    assert lib.kvq_ce_forward_stats_ignore(one, one, big, 8, 0, one, 1, 0, one, one, one, None, None, None, None) != 0
    assert lib.kvq_ce_backward_ignore(one, one, one, None, one, 0, big, 8, 8, 0, one, None) != 0
    assert lib.kvq_ce_backward_bias_ignore(one, one, one, None, one, 0, big, 8, 8, 0, one, one, 1 << 40, None) != 0
    assert lib.kvq_ce_backward_ignore(one, one, one, None, None, 0, 9, 8, 8, 0, one, None) != 0          # count is required
    assert b"null pointer" in lib.kvq_last_error()
    assert lib.kvq_ce_backward_bias_ignore(one, one, one, None, None, 0, 9, 8, 8, 0, one, one, 1 << 20, None) != 0
    assert lib.kvq_seq_acc_ignore(None, one, 5, 12, 0, one, None) != 0


# ---- the nnops wrappers that pick the entry point -----------------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) before the arguments were checked")


def test_loss_wrappers_check_ignore_index_and_count_before_the_library(monkeypatch):
    """ignore_index and count go together: a count without an ignore_index is refused by every wrapper that takes one, an
    ignore_index without a count by the backward ones (their entry points read it), and an ignore_index that is no int by all --
    on CPU tensors, with the library out of reach."""
    from kvq import nnops
    from kvq._ffi import KvqError
    monkeypatch.setattr(nnops, "lib", lambda: _NoLibrary())
    N, V = 4, 8
    x = torch.zeros(N, V); t = torch.zeros(N, dtype=torch.int64); f = torch.zeros(N); p = torch.zeros(N, dtype=torch.int64)
    s = torch.zeros(1); part = torch.zeros(1, V); stats = torch.zeros(N, 1, 4)
    calls = {
        "ce_forward": lambda **kw: nnops.ce_forward(x, t, V, V, f, f, p, s, s, **kw),
        "ce_forward_stats": lambda **kw: nnops.ce_forward_stats(x, t, stats, f, f, p, s, s, **kw),
        "ce_backward": lambda **kw: nnops.ce_backward(x, t, f, s, V, V, x, **kw),
        "ce_backward_bias": lambda **kw: nnops.ce_backward_bias(x, t, f, s, V, V, x, part, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(KvqError, match=name + ": count"):
            call(ignore_index=None, count=s)
        for bad in (True, 0.0, "0", s):
            with pytest.raises(KvqError, match=name + ": ignore_index must be"):
                call(ignore_index=bad, count=s)
    for name in ("ce_backward", "ce_backward_bias"):
        with pytest.raises(KvqError, match=name + ": ignore_index=-100 needs the count"):
            calls[name](ignore_index=-100, count=None)
    with pytest.raises(KvqError, match="seq_acc: ignore_index must be"):
        nnops.seq_acc(p, t, 2, 2, torch.zeros(2), ignore_index=False)
    for args in ((p, t, 2, 3, torch.zeros(2)), (p, t[:3], 2, 2, torch.zeros(2)), (p, t, 2, 2, torch.zeros(3))):
        with pytest.raises(KvqError, match="seq_acc: pred and target must hold"):
            nnops.seq_acc(*args, ignore_index=0)
