"""Host-side checks of the fp8 input-gradient option: the new entry points refuse bad arguments before any HIP call (error code and
message, no crash), the ctypes table knows them, both entry-point configurations carry FP8_BACKWARD."""
import ctypes
import importlib
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")


def _lib():
    from kvq import _ffi
    return _ffi.lib()


def test_format_constants_and_signatures():
    from kvq import _ffi
    assert (_ffi.FP8_E4M3, _ffi.FP8_E5M2) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "kvq.h")).read()
    assert "#define KVQ_FP8_E4M3 0" in hdr and "#define KVQ_FP8_E5M2 1" in hdr
    for name in ("kvq_gemm_fp8_nt_ex", "kvq_fp8_quantize_fmt", "kvq_fp8_quantize_delayed_fmt", "kvq_fp8_update_scales_fmt",
                 "kvq_fp8_transpose", "kvq_fp8_transpose_segments"):
        assert name in _ffi.SIGNATURES and hasattr(_lib(), name)


def test_gemm_entry_refuses_before_any_launch():
    lib = _lib()
    p = 4096                                           # a 16-byte aligned address that is never read: every call below is refused first
    args = lambda M, N, K, lda, ldb, ldc, fmt, acc: (p, p, p, p, None, p, M, N, K, lda, ldb, ldc, fmt, acc, None)
    assert lib.kvq_gemm_fp8_nt_ex(*args(256, 64, 192, 192, 192, 64, 1, 0)) == -1 and b"K % 128" in lib.kvq_last_error()
    assert lib.kvq_gemm_fp8_nt_ex(*args(256, 64, 128, 136, 128, 64, 1, 0)) == -1 and b"lda, ldb % 16" in lib.kvq_last_error()
    assert lib.kvq_gemm_fp8_nt_ex(*args(256, 64, 128, 128, 128, 64, 2, 0)) == -1 and b"a_format" in lib.kvq_last_error()
    assert lib.kvq_gemm_fp8_nt_ex(p, p, None, p, None, p, 256, 64, 128, 128, 128, 64, 1, 1, None) == -1 and b"scale" in lib.kvq_last_error()
    assert lib.kvq_gemm_fp8_nt_ex(*args(256, 60, 128, 128, 128, 64, 1, 1)) == -1 and b"multiples of 8" in lib.kvq_last_error()


def test_transpose_and_quantise_entries_refuse_before_any_launch():
    lib = _lib()
    p = 4096
    assert lib.kvq_fp8_transpose(p, 24, 32, 32, p, 32, None) == -1 and b"multiples of 16" in lib.kvq_last_error()
    assert lib.kvq_fp8_transpose(p, 32, 24, 32, p, 32, None) == -1 and b"multiples of 16" in lib.kvq_last_error()
    assert lib.kvq_fp8_transpose(p, 32, 32, 16, p, 32, None) == -1                       # a row stride shorter than the row
    assert lib.kvq_fp8_transpose(p + 8, 32, 32, 32, p, 32, None) == -1 and b"aligned" in lib.kvq_last_error()
    assert lib.kvq_fp8_transpose(None, 32, 32, 32, p, 32, None) == -1
    assert lib.kvq_fp8_transpose_segments(p, p, p, p, p, None, 3, 4, None) == -1
    assert lib.kvq_fp8_transpose_segments(p, p, p, p, p, p, 0, 4, None) == -1
    assert lib.kvq_fp8_transpose_segments(p, p, p, p, p, p, 3, 0, None) == -1
    assert lib.kvq_fp8_quantize_fmt(p, 16, 16, 16, p, p, p, 7, None) == -1 and b"fmt" in lib.kvq_last_error()
    assert lib.kvq_fp8_quantize_fmt(p, 16, 12, 16, p, p, p, 1, None) == -1
    assert lib.kvq_fp8_quantize_delayed_fmt(p, 16, 16, 8, None, p, 1, None) == -1        # ld < cols
    assert lib.kvq_fp8_quantize_delayed_fmt(p, 16, 16, 16, p, None, 1, None) == -1
    assert lib.kvq_fp8_update_scales_fmt(p, 1, 0.5, 1, None) == -1 and b"headroom" in lib.kvq_last_error()
    assert lib.kvq_fp8_update_scales_fmt(p, 1, 4.0, 3, None) == -1


@pytest.mark.parametrize("model", ["shelgon3", "bagon"])
def test_config_carries_fp8_backward(model):
    sys.path.insert(0, os.path.join(PKG, "models", model))
    try:
        sys.modules.pop("config", None)
        cfg = importlib.import_module("config")
        assert cfg.FP8_BACKWARD is False and cfg.get_config()["fp8_backward"] is False
        main = open(os.path.join(PKG, "models", model, "main.py")).read()
        assert "fp8_backward=FP8_BACKWARD" in main
    finally:
        sys.path.pop(0)
        sys.modules.pop("config", None)
