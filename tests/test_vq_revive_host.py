"""Host-side checks of the codebook revival (VectorQuantizer(revive_after=...)): include/kvq.h declares the
three entry points and the counter, the ctypes table knows them, every bad argument is refused before any HIP call, the Shelgon
configuration carries VQ_REVIVE_AFTER and honours KVQ_VQ_REVIVE_AFTER, the modules carry state only with the option set, and the
numpy restatement's Philox4x32-10 reproduces the known-answer vectors."""
import importlib
import os
import re
import sys

import pytest

import _revive_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")
ENTRY_POINTS = ("kvq_vq_usage_flags", "kvq_vq_revive_select", "kvq_vq_revive_apply")


def _config():
    sys.path.insert(0, os.path.join(PKG, "models", "shelgon3"))
    try:
        sys.modules.pop("config", None)
        return importlib.import_module("config")
    finally:
        sys.path.pop(0)
        sys.modules.pop("config", None)


def test_philox_known_answers():
    assert R.philox4x32(0, 0, 0, 0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    f = 0xFFFFFFFF
    assert R.philox4x32(f, f, f, f, f, f) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    for seed, c, N, world in ((0, 0, 1, 1), (12345, 7, 70, 4), (2**63 + 5, 2**31 - 1, 2**32 - 1, 3)):
        owner, n = R.draw(seed, c, N, world)
        assert 0 <= owner < world and 0 <= n < N


def test_header_declares_the_entry_points_and_the_ctypes_table_knows_them():
    from kvq import _ffi
    hdr = open(os.path.join(ROOT, "include", "kvq.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _ffi.lib()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert name in _ffi.SIGNATURES and hasattr(lib, name)
    assert "struct { uint32_t last, pad; uint64_t total; }" in hdr
    assert "0x52455649" in hdr and "%x" % R.SITE == "52455649"
    src = open(os.path.join(PKG, "csrc", "kvq_vq_revive.hip")).read()
    assert "hipMemsetAsync" not in src and "hipMemcpy" not in src and "atomicAdd" not in src         # kernels only, no float atomics


def test_entry_points_refuse_before_any_launch():
    from kvq import _ffi
    lib = _ffi.lib()
    p = 4096                                                    # an aligned address that is never read: every call below is refused first
    err = lib.kvq_last_error
    # usage flags
    assert lib.kvq_vq_usage_flags(None, 8, 4, 1, p, None) == -1 and b"kvq_vq_usage_flags" in err()
    assert lib.kvq_vq_usage_flags(p, 8, 4, 1, None, None) == -1
    for N, K, G in ((0, 4, 1), (8, 0, 1), (8, 4, 0), (-1, 4, 1)):
        assert lib.kvq_vq_usage_flags(p, N, K, G, p, None) == -1 and b">= 1" in err(), (N, K, G)
    assert lib.kvq_vq_usage_flags(p, 2**32, 4, 1, p, None) == -1 and b"2^32" in err()
    # select: (z, used, N, K, D, G, io_dtype, revive_after, seed, rank, world, idle, rows, stream)
    good = dict(z=p, used=p, N=8, K=4, D=8, G=1, dt=1, T=2, seed=1, rank=0, world=1, idle=p, rows=p)

    def select(**kw):
        a = dict(good, **kw)
        return lib.kvq_vq_revive_select(a["z"], a["used"], a["N"], a["K"], a["D"], a["G"], a["dt"], a["T"], a["seed"], a["rank"], a["world"],
                                        a["idle"], a["rows"], None)
    for name in ("z", "used", "idle", "rows"):
        assert select(**{name: None}) == -1 and b"null pointer" in err(), name
    for name in ("N", "K", "D", "G"):
        assert select(**{name: 0}) == -1 and b">= 1" in err(), name
        assert select(**{name: -3}) == -1, name
    assert select(N=2**32) == -1 and b"2^32" in err()
    assert select(N=2**32 + 5) == -1
    for T in (0, -1):
        assert select(T=T) == -1 and b"revive_after" in err()
    for world in (0, -2):
        assert select(world=world) == -1 and b"world" in err()
    for rank, world in ((-1, 1), (1, 1), (4, 4), (7, 2)):
        assert select(rank=rank, world=world) == -1 and b"rank" in err(), (rank, world)
    for dt in (2, -1, 7):
        assert select(dt=dt) == -1 and b"dtype" in err()
    assert select(z=p + 8) == -1 and b"aligned" in err()
    assert select(rows=p + 4) == -1 and b"aligned" in err()
    # apply: (rows, K, D, G, revive_after, idle, E, m, v, vmax, ema_n, ema_m, counter, stream)
    goodA = dict(rows=p, K=4, D=8, G=1, T=2, idle=p, E=p, counter=p)

    def apply(**kw):
        a = dict(goodA, **kw)
        return lib.kvq_vq_revive_apply(a["rows"], a["K"], a["D"], a["G"], a["T"], a["idle"], a["E"], None, None, None, None, None,
                                       a["counter"], None)
    for name in ("rows", "idle", "E", "counter"):
        assert apply(**{name: None}) == -1 and b"null pointer" in err(), name
    for name in ("K", "D", "G"):
        assert apply(**{name: 0}) == -1 and b">= 1" in err(), name
    assert apply(T=0) == -1 and b"revive_after" in err()
    assert apply(rows=p + 8) == -1 and b"aligned" in err()
    assert apply(E=p + 4) == -1 and b"aligned" in err()


def test_config_carries_revive_after_and_honours_the_environment(monkeypatch):
    monkeypatch.delenv("KVQ_VQ_REVIVE_AFTER", raising=False)
    cfg = _config()
    assert cfg.VQ_REVIVE_AFTER is None and cfg.get_config()["vq_revive_after"] is None
    for text, want in (("100", 100), ("1", 1), ("", None)):
        monkeypatch.setenv("KVQ_VQ_REVIVE_AFTER", text)
        cfg = _config()
        assert cfg.VQ_REVIVE_AFTER == want and cfg.get_config()["vq_revive_after"] == want, text
    for bad in ("0", "-3", "2.5", "soon", "True"):
        monkeypatch.setenv("KVQ_VQ_REVIVE_AFTER", bad)
        with pytest.raises(ValueError, match="VQ_REVIVE_AFTER"):
            _config()
    main = open(os.path.join(PKG, "models", "shelgon3", "main.py")).read()
    assert main.count("revive_after=VQ_REVIVE_AFTER") == 2 and '"vq_revive_after"' in main        # both constructors, run_conf.json
    trainer = open(os.path.join(PKG, "models", "shelgon3", "Trainer.py")).read()
    assert "codes_revived" in trainer and "revive_epoch_record" in trainer


def test_engine_option_validation_needs_no_device(monkeypatch):
    from kvq._ffi import KvqError
    from kvq.functional import check_revive_after as check
    monkeypatch.delenv("KVQ_VQ_REVIVE_AFTER", raising=False)
    assert check(None) is None and check(None, env=True) is None
    assert check(1) == 1 and check(100) == 100
    for bad in (0, -1, 2.0, "3", True, [3], 2**31):
        with pytest.raises(KvqError, match="revive_after"):
            check(bad)
    monkeypatch.setenv("KVQ_VQ_REVIVE_AFTER", "")
    assert check(None, env=True) is None
    monkeypatch.setenv("KVQ_VQ_REVIVE_AFTER", "100")
    assert check(None, env=True) == 100 and check(None) is None and check(7, env=True) == 7
    for bad in ("0", "-1", "1.5", "soon"):
        monkeypatch.setenv("KVQ_VQ_REVIVE_AFTER", bad)
        with pytest.raises(KvqError, match="revive_after"):
            check(None, env=True)


def test_modules_carry_state_only_with_the_option():
    import torch
    from models.shelgon3.MultiVectorQuantizer import MultiVectorQuantizer
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    vq = VectorQuantizer(16, 32, 0.25)
    assert vq.revive_after is None and list(vq.buffers()) == [] and list(vq.state_dict()) == ["embedding.weight"]
    with pytest.raises(RuntimeError, match="revive_after"):
        vq.revive(torch.zeros(4, 32), torch.zeros(4, dtype=torch.int64))
    mq = MultiVectorQuantizer(2, 16, 32, 0.25)
    assert mq.revive_after is None and list(mq.state_dict()) == ["embedding.weight"]
    assert sorted(n for n, _ in mq.named_buffers()) == ["col_map", "inv_map"]                      # what it had before, not persistent

    vq = VectorQuantizer(16, 32, 0.25, revive_after=3)
    assert vq.revive_after == 3 and vq.code_idle.shape == (16,) and vq.code_idle.dtype == torch.int32 and not vq.code_idle.any()
    assert vq.revive_counter.dtype == torch.int64 and vq.revive_counter.numel() == 2               # the 16-byte counter
    assert sorted(vq.state_dict()) == ["code_idle", "embedding.weight"]
    vq.code_idle.copy_(torch.arange(16, dtype=torch.int32))
    other = VectorQuantizer(16, 32, 0.25, revive_after=3)
    other.load_state_dict(vq.state_dict())
    assert torch.equal(other.code_idle, torch.arange(16, dtype=torch.int32)) and other.code_idle.dtype == torch.int32
    assert torch.equal(other.embedding.weight, vq.embedding.weight)

    mq = MultiVectorQuantizer(2, 16, 32, 0.25, ema_decay=0.99, revive_after=5)
    assert mq.code_idle.shape == (2, 16) and mq.code_idle.dtype == torch.int32
    assert sorted(mq.state_dict()) == ["code_idle", "ema_m", "ema_n", "embedding.weight"]
    for bad in (0, -1, 2.5, "3", True):
        with pytest.raises(Exception, match="revive_after"):
            VectorQuantizer(16, 32, 0.25, revive_after=bad)


def test_restatement_of_one_step():
    """The restatement against a hand-worked case: which codes die, saturation of idle, what apply touches."""
    import numpy as np
    idx = np.array([[0, 2, 2, -1, 5, 1]], np.int64)                         # K = 5: -1 and 5 are ignored
    used = R.usage_flags(idx, 5)
    assert used.tolist() == [[1, 1, 1, 0, 0]]
    idle = np.array([[7, 0, R.INT32_MAX, 1, R.INT32_MAX]], np.int32)
    z = np.arange(6 * 3, dtype=np.float32).reshape(1, 6, 3) - 4.0
    idle2, dead, rows, owner, token = R.select([z], used, idle, 2, seed=99)
    assert idle2.tolist() == [[0, 0, 0, 2, R.INT32_MAX]] and dead.tolist() == [[False, False, False, True, True]]
    for k in (3, 4):
        assert owner[0, k] == 0 and token[0, k] == R.draw(99, k, 6)[1] and np.array_equal(rows[0, k], z[0, token[0, k]])
    E = np.ones((1, 5, 3), np.float32)
    m = np.full((1, 5, 3), 2.0, np.float32)
    ema_n = np.full((1, 5), 9.0, np.float32)
    idle3, E2, counter, opt = R.apply(rows, dead, idle2, E, (0, 10), m=m, ema_n=ema_n)
    assert idle3.tolist() == [[0, 0, 0, 0, 0]] and counter == (2, 12)
    assert np.array_equal(E2[0, :3], E[0, :3]) and np.array_equal(E2[0, 3:], rows[0, 3:])
    assert opt["m"][0, :3].min() == 2.0 and not opt["m"][0, 3:].any() and opt["ema_n"].tolist() == [[9.0, 9.0, 9.0, 1.0, 1.0]]
    assert opt["v"] is None and opt["ema_m"] is None
