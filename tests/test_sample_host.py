"""Host side of top-k / top-p sampling, no GPU: the ctypes signature of kvq_gen_select_filtered against include/kvq.h, the words of
the filter state, and every refusal of generate / generate_codes / beam_search / traverse_codes and of the analysis switches that
needs no device."""
import os
import re
import struct
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")


def test_ffi_table_binds_the_filtered_selection_with_the_headers_arity():
    from kvq import _ffi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kvq.h")).read(), flags=re.S)
    name = "kvq_gen_select_filtered"
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
    assert m, f"{name} is not declared in include/kvq.h"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _ffi.SIGNATURES[name]
    assert res is _ffi._int and len(args) == len(params) == 15
    for p, a in zip(params, args):
        want = _ffi._vp if "*" in p else (_ffi._i64 if p.startswith("int64_t") else _ffi._int)
        assert a is want, (name, p)
    assert [p.split()[-1].lstrip("*") for p in params] == ["state", "filter", "logits", "ld", "V", "B", "io_dtype", "ids", "finished", "lengths",
                                                           "step_logits", "step_kept", "step_cut", "step_logprob", "stream"]
    lib = _ffi.lib()
    assert getattr(lib, name)(*[None if a is _ffi._vp else 0 for a in args]) == -1 and b"kvq_gen_select_filtered" in lib.kvq_last_error()
    # the contract stands in the header: order, tie rule, the HuggingFace cut, the filter state, the derived bounds
    header = open(os.path.join(ROOT, "include", "kvq.h")).read()
    for text in ("struct { int32 top_k; float top_p; int32 reserved[2]; }", "y_v == y_w and v < w", "TopPLogitsWarper", "TOL_MASS = 2^-17",
                 "V <= 32768"):
        assert text in header, text


def test_filter_words_and_what_a_filter_state_refuses():
    from kvq import nnops
    from kvq._ffi import KvqError
    assert nnops.gen_filter_words() == [0, 0x3F800000, 0, 0]
    assert nnops.gen_filter_words(50, 0.5) == [50, 0x3F000000, 0, 0]
    w = nnops.gen_filter_words(7, 0.9)
    assert struct.unpack("<f", struct.pack("<i", w[1]))[0] == struct.unpack("<f", struct.pack("<f", 0.9))[0] and w[2:] == [0, 0]
    assert nnops.gen_filter_words(top_k=(1 << 31) - 1)[0] == (1 << 31) - 1
    st = nnops.new_gen_filter("cpu", 3, 0.25)
    assert st.dtype == torch.int32 and st.tolist() == [3, 0x3E800000, 0, 0] and st.numel() * st.element_size() == 16
    for bad in (dict(top_k=-1), dict(top_k=1.0), dict(top_k=True), dict(top_k=1 << 31), dict(top_k=None), dict(top_p=0.0), dict(top_p=-0.1),
                dict(top_p=1.5), dict(top_p=float("nan")), dict(top_p=float("inf")), dict(top_p="0.5"), dict(top_p=True), dict(top_p=None)):
        with pytest.raises(KvqError, match="top_k" if "top_k" in bad else "top_p"):
            nnops.gen_filter_words(**bad)
    assert nnops.GEN_FILTER_MAX_V == 32768
    z32 = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(KvqError):                                                 # CPU tensors: there is no CPU path
        nnops.gen_select_filtered(torch.zeros(8, dtype=torch.int32), st, torch.zeros(2, 8), 8, torch.zeros((2, 4), dtype=torch.int64), z32, z32)


def test_generate_refuses_bad_filters_without_a_device():
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    check = lambda k=0, p=1.0, tau=1.0, scores=False, V=2048: TrainEngine._check_filters(k, p, tau, scores, V)
    assert check() is False and check(tau=0.0) is False                           # filters off: today's call
    assert check(k=5) is True and check(p=0.9) is True and check(k=5, p=0.5, tau=0.3) is True
    assert check(scores=True) is True and check(scores=True, tau=0.0) is True     # the score of the greedy sentence is allowed
    assert check(k=4096) is True and check(p=1) is False
    for kw, text in ((dict(k=-1), "top_k"), (dict(k=2.0), "top_k"), (dict(k=True), "top_k"), (dict(k="5"), "top_k"), (dict(k=None), "top_k"),
                     (dict(p=0.0), "top_p"), (dict(p=-0.5), "top_p"), (dict(p=1.0001), "top_p"), (dict(p=float("nan")), "top_p"),
                     (dict(p=float("inf")), "top_p"), (dict(p=None), "top_p"), (dict(p=True), "top_p"),
                     (dict(k=5, tau=0.0), "temperature 0"), (dict(p=0.5, tau=0.0), "temperature 0"), (dict(k=5, p=0.5, tau=0), "temperature 0"),
                     (dict(k=5, V=32769), "vocabulary"), (dict(scores=True, V=119547), "vocabulary")):
        with pytest.raises(KvqError, match=text):
            check(**kw)
    assert check(V=119547) is False                                               # the unfiltered call has no capacity limit


def test_beam_search_refuses_the_sampling_keys_by_name_with_a_kvq_error():
    from kvq._ffi import KvqError
    from kvq.engine import TrainEngine
    for key, value in (("top_k", 5), ("top_p", 0.9), ("temperature", 1.0), ("seed", 3), ("want_scores", True), ("temperature", 0.0), ("top_k", 0)):
        for who in ("beam_search", "beam_search_codes"):
            with pytest.raises(KvqError, match=key):
                TrainEngine._refuse_sampling(who, {key: value})
    with pytest.raises(KvqError, match="top_k, top_p"):
        TrainEngine._refuse_sampling("beam_search", dict(top_p=0.5, top_k=3))
    with pytest.raises(TypeError, match="unexpected keyword"):
        TrainEngine._refuse_sampling("beam_search", dict(no_such=1))
    TrainEngine._refuse_sampling("beam_search", {})
    with pytest.raises(TypeError, match="temperature"):                           # ... and still the TypeError an unknown keyword is
        TrainEngine._refuse_sampling("beam_search", dict(temperature=1.0))
    # the public methods run the refusal first: before _latent_call, before anything that needs an engine
    fake = SimpleNamespace(_refuse_sampling=TrainEngine._refuse_sampling, _SAMPLING_KEYS=TrainEngine._SAMPLING_KEYS)
    with pytest.raises(KvqError, match="want_scores"):
        TrainEngine.beam_search(fake, None, 8, None, 2, want_scores=True)
    with pytest.raises(KvqError, match="seed"):
        TrainEngine.beam_search_codes(fake, None, 8, None, 2, seed=1)


def test_model_methods_hand_the_sampling_keys_to_the_engine():
    """num_beams == 1: generate / generate_codes receive them; num_beams > 1: beam_search receives them (and refuses them there)"""
    import kvq.engine as E
    from models.bagon.Bagon import Bagon
    from models.shelgon3.Shelgon import Shelgon
    calls = []

    class Stub:
        def __getattr__(self, name):
            return lambda *a, **kw: calls.append((name, a, kw)) or {}

    old = E.engine_of
    E.engine_of = lambda model: Stub()
    try:
        Bagon.generate_from_latents(object(), "z", 8, "p", temperature=0.7, top_k=5, top_p=0.9, seed=2, want_scores=True)
        assert calls[-1] == ("generate", ("z", 8, "p"), dict(temperature=0.7, top_k=5, top_p=0.9, seed=2, want_scores=True))
        Bagon.generate_from_latents(object(), "z", 8, "p", num_beams=3, top_k=5)
        assert calls[-1] == ("beam_search", ("z", 8, "p", 3), dict(length_penalty=0.0, top_k=5))
        Shelgon.generate_from_codes(object(), "i", 8, "p", top_p=0.5, temperature=1.0)
        assert calls[-1] == ("generate_codes", ("i", 8, "p"), dict(top_p=0.5, temperature=1.0))
        Shelgon.generate_from_codes(object(), "i", 8, "p", num_beams=2, want_scores=True)
        assert calls[-1] == ("beam_search_codes", ("i", 8, "p", 2), dict(length_penalty=0.0, want_scores=True))
        Shelgon.traverse_codes(object(), "e", "m", 1, 2, free_running=True, temperature=0.8, seed=4, top_k=3, top_p=0.6, want_scores=True)
        name, a, kw = calls[-1]
        assert name == "traverse_codes" and a == ("e", "m", 1, 2)
        assert {k: kw[k] for k in ("free_running", "temperature", "seed", "top_k", "top_p", "want_scores")} == dict(
            free_running=True, temperature=0.8, seed=4, top_k=3, top_p=0.6, want_scores=True)
    finally:
        E.engine_of = old


def test_analysis_switches_parse_the_command_line_and_refuse_samples_with_beams():
    sys.path.insert(0, PKG)
    from analyses.latent_arithmetics import latent_arithmetics as LA
    from analyses.latent_traversals import code_traversal as CT
    for mod in (LA, CT):
        assert (mod.SAMPLES, mod.TEMPERATURE, mod.TOP_K, mod.TOP_P, mod.SEED, mod.NUM_BEAMS) == (0, 1.0, 0, 1.0, 0, 1)
    old = sys.argv
    try:
        sys.argv = ["x"]
        assert LA.sampling_switch(0, 1.0, 0, 1.0, 0) == dict(samples=0, temperature=1.0, top_k=0, top_p=1.0, seed=0)
        sys.argv = ["x", "--free-running", "--samples", "2", "--top-k", "5", "--top-p", "0.9", "--temperature", "0.7", "--seed", "11"]
        assert LA.sampling_switch(0, 1.0, 0, 1.0, 0) == dict(samples=2, temperature=0.7, top_k=5, top_p=0.9, seed=11)
        assert CT.sampling_switch is LA.sampling_switch
        with pytest.raises(SystemExit, match="num-beams"):
            LA.sampling_switch(0, 1.0, 0, 1.0, 0, num_beams=2)
        sys.argv = ["x", "--samples", "-1"]
        with pytest.raises(SystemExit, match="samples"):
            LA.sampling_switch(0, 1.0, 0, 1.0, 0)
        sys.argv = ["x"]
        assert LA.sampling_switch(3, 0.5, 4, 0.8, 9)["samples"] == 3             # the configured constants
        with pytest.raises(SystemExit, match="num-beams"):
            LA.sampling_switch(3, 0.5, 4, 0.8, 9, num_beams=4)
    finally:
        sys.argv = old
    tok = SimpleNamespace(batch_decode=lambda ids: ["s" + "".join(str(int(i)) for i in row) for row in ids])
    assert LA.sample_columns(tok, 1, torch.tensor([1, 2]), torch.tensor(-1.5, dtype=torch.float64), "edited_") == {
        "edited_sample_1": "s12", "edited_sample_1_score": -1.5}
