"""The CPU oracle (oracle/) against the golden vectors produced by the reference's own VectorQuantizer.

This is what pins the oracle: every other parity test compares the HIP path with the oracle.
"""
import json
import os

import numpy as np
import pytest

from _golden_util import GOLDEN, case_names, check_flip_budget, check_indices, load_case
from oracle import vq_oracle as O

CASES = case_names()


@pytest.fixture(scope="module", autouse=True)
def _build():
    O.build()


@pytest.mark.parametrize("name", CASES)
def test_c_oracle_forward_matches_reference(name):
    c = load_case(name)
    out = O.vq_forward(c["z"], c["E"], float(c["beta"]))
    ndiff = check_indices(c, out["idx"])
    check_flip_budget(c, ndiff)
    if c["regime"] in ("separated", "onto_codes", "ties"):
        assert ndiff == 0, f"{name}: {ndiff} index mismatches on a well-separated case"
    if ndiff == 0:
        # z_q is a pure function of (z, E, idx): bitwise equal to the reference  (VectorQuantizer.py:72,:80)
        import hashlib
        assert hashlib.sha256(out["z_q"].tobytes()).hexdigest() == c["sha_zq"]
        if c["full"]:
            assert np.array_equal(out["z_q"], c["z_q"])
        np.testing.assert_allclose(out["perplexity"], c["perplexity"], rtol=2e-5)
    # loss differs from the reference only by summation order of the mean
    np.testing.assert_allclose(out["loss"], c["loss"], rtol=2e-6, atol=1e-12)
    assert out["counts"].sum() == c["B"] * c["S"]


@pytest.mark.parametrize("name", CASES)
def test_c_oracle_backward_matches_reference(name):
    c = load_case(name)
    # use the reference's own indices so that near-tie flips do not leak into the gradient check
    gz, gE = O.vq_backward(c["z"], c["E"], c["idx"], c["g"], float(c["c"]), float(c["beta"]))
    D = c["D"]
    if c["full"]:
        np.testing.assert_allclose(gz, c["grad_z"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(gE, c["grad_E"], rtol=2e-5, atol=1e-7)
    else:
        np.testing.assert_allclose(gz.reshape(-1, D)[c["tok_rows"]], c["grad_z_rows"], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(gE[c["code_rows"]], c["grad_E_rows"], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(gz.astype(np.float64).sum(), c["grad_z_sum"], rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose((gz.astype(np.float64) ** 2).sum(), c["grad_z_sq"], rtol=1e-5)
    np.testing.assert_allclose((gE.astype(np.float64) ** 2).sum(), c["grad_E_sq"], rtol=1e-4, atol=1e-12)
    # codes nobody chose get exactly zero gradient
    unused = np.setdiff1d(np.arange(c["K"]), c["idx"])
    assert not gE[unused].any()


def test_c_oracle_large_codebook_near_ties():
    """BASELINE.json configs[3] where index parity is hardest: K = 8192 with the reference's default codebook init
    (models/shelgon3/VectorQuantizer.py:29,59-65) at N = 8192 -- 5310 tokens whose two best codes are closer than 1e-3, and the
    reference's f32 arg-min itself differs from fp64 on 124 of them.  The oracle (all host threads; it is the same arithmetic
    per token) must reproduce the reference's choice within the recorded flip budget."""
    import hashlib
    import os
    c = load_case("k8192_default")
    assert int((c["gap64"] < 1e-3).sum()) > 5000 and int((c["idx"] != c["idx64"]).sum()) == 124
    O.set_threads(os.cpu_count() or 1)
    try:
        out = O.vq_forward(c["z"], c["E"], float(c["beta"]))
        gz, gE = O.vq_backward(c["z"], c["E"], c["idx"], c["g"], float(c["c"]), float(c["beta"]))
    finally:
        O.set_threads(1)
    ndiff = check_indices(c, out["idx"])
    check_flip_budget(c, ndiff)
    np.testing.assert_allclose(out["loss"], c["loss"], rtol=2e-6)
    if ndiff == 0:
        assert hashlib.sha256(out["z_q"].tobytes()).hexdigest() == c["sha_zq"]
        np.testing.assert_allclose(out["perplexity"], c["perplexity"], rtol=2e-5)     # 5100 codes in use: needs the f64 sum
    D = c["D"]
    np.testing.assert_allclose(gz.reshape(-1, D)[c["tok_rows"]], c["grad_z_rows"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(gE[c["code_rows"]], c["grad_E_rows"], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose((gE.astype(np.float64) ** 2).sum(), c["grad_E_sq"], rtol=1e-4)


TORCH_EXPR_CASES = [n for n in CASES if not n.startswith("k8192")]


def _torch_expr_restatement(name):
    """oracle.vq_oracle.torch_expr_forward on case `name`, forward and backward, as numpy arrays."""
    import torch
    torch.set_num_threads(1)
    c = load_case(name)
    w = torch.from_numpy(c["E"].copy()).requires_grad_(True)
    z = torch.from_numpy(c["z"].copy()).requires_grad_(True)
    loss, z_q, perp, enc, idx = O.torch_expr_forward(z, w, float(c["beta"]))
    (float(c["c"]) * loss + (z_q * torch.from_numpy(c["g"])).sum()).backward()
    return dict(idx=idx.numpy(), loss=np.float32(loss.item()), perplexity=np.float32(perp.item()), enc_shape=np.array(enc.shape),
                grad_z=z.grad.numpy(), grad_E=w.grad.numpy())


@pytest.fixture(scope="module")
def torch_expr_results(tmp_path_factory):
    """Every case's restatement, computed in one child process with MKL's code branch pinned to COMPATIBLE (MKL_CBWR), as
    tests/golden/vq_perplexity_pinned.json was recorded: MKL's vector-math log rounds differently on different CPUs otherwise,
    and this process's MKL has chosen its branch long before."""
    import subprocess
    import sys
    out = tmp_path_factory.mktemp("torch_expr")
    code = (f"import sys; sys.path[:0] = {sys.path!r}\n"
            "import numpy as np, test_oracle_golden as t\n"
            f"for n in {TORCH_EXPR_CASES!r}:\n"
            f"    np.savez({str(out)!r} + '/' + n + '.npz', **t._torch_expr_restatement(n))\n")
    flags = ["-s"] if sys.flags.no_user_site else []
    subprocess.run([sys.executable, *flags, "-c", code], env=dict(os.environ, MKL_CBWR="COMPATIBLE"), check=True, timeout=600)
    return lambda name: np.load(out / f"{name}.npz")


@pytest.mark.parametrize("name", TORCH_EXPR_CASES)
def test_torch_expr_restatement_matches_reference(name, torch_expr_results):
    """The expression-for-expression torch restatement is the reference's op sequence: identical results.  The perplexity is
    compared with the reference's under the same MKL pin (tests/golden/vq_perplexity_pinned.json); loss, indices and gradients
    do not depend on the pin on these cases."""
    c = load_case(name)
    r = torch_expr_results(name)
    idx = r["idx"]
    with open(os.path.join(GOLDEN, "vq_perplexity_pinned.json")) as f:
        pinned_perplexity = np.float32(json.load(f)[name])
    assert np.array_equal(idx.reshape(-1), c["idx"])
    assert r["loss"] == c["loss"] and r["perplexity"] == pinned_perplexity
    if c["full"]:
        assert np.array_equal(r["grad_z"], c["grad_z"]) and np.array_equal(r["grad_E"], c["grad_E"])
    assert tuple(r["enc_shape"]) == (c["B"] * c["S"], c["K"]) and idx.shape == (c["B"], c["S"], 1)


def test_tie_rule_first_index_wins():
    """Hand-made tie (SURVEY.md §8c golden item 3): duplicated codebook rows -> the lowest index is chosen."""
    c = load_case("tiny_ties")
    K = c["K"]
    out = O.vq_forward(c["z"], c["E"], 0.25)
    assert (out["idx"] < K - K // 2).all()
    # exact duplicates of the winner exist at idx + K//2: distances are bitwise equal there
    d = O.distances(c["z"], c["E"])
    n = np.arange(d.shape[0])
    assert np.array_equal(d[n, out["idx"]], d[n, out["idx"] + K // 2])


def test_known_answer_identities():
    """loss == (1+beta)*mean((E[idx]-z)^2); perplexity == exp(-sum p log(p+1e-10)); z_q == z+(E[idx]-z) bitwise."""
    rng = np.random.default_rng(11)
    z = rng.standard_normal((3, 9, 24), dtype=np.float32)
    E = rng.standard_normal((13, 24), dtype=np.float32)
    out = O.vq_forward(z, E, 0.4)
    e = E[out["idx"]].reshape(z.shape)
    assert np.array_equal(out["z_q"], z + (e - z))
    np.testing.assert_allclose(out["loss"], 1.4 * np.mean((e.astype(np.float64) - z) ** 2), rtol=1e-6)
    p = np.bincount(out["idx"], minlength=13) / 27.0
    np.testing.assert_allclose(out["perplexity"], np.exp(-(p * np.log(p + 1e-10)).sum()), rtol=1e-5)
    # nan rule of torch.argmin: a NaN distance wins
    z2 = z.copy(); z2[0, 0, 0] = np.nan
    assert O.vq_forward(z2, E, 0.4)["idx"][0] == 0


def test_oracle_dot_order_is_documented_walk():
    """kvq order v1: groups of 8 visited 0,4,1,5,2,6,3,7 as one fmaf chain."""
    import ctypes as C
    import math
    lib = O.load()
    rng = np.random.default_rng(5)
    for D in (8, 16, 40, 13):
        a = rng.standard_normal(D).astype(np.float32); b = rng.standard_normal(D).astype(np.float32)
        acc = np.float32(0)
        for g in range((D + 7) // 8):
            for s in range(8):
                j = 8 * g + (s >> 1) + ((s & 1) << 2)
                if j < D:
                    acc = np.float32(math.fma(float(a[j]), float(b[j]), float(acc))) if hasattr(math, "fma") else \
                        np.float32(np.float64(a[j]) * np.float64(b[j]) + np.float64(acc))
        got = lib.kvq_oracle_dot(a.ctypes.data_as(C.POINTER(C.c_float)), b.ctypes.data_as(C.POINTER(C.c_float)), D)
        assert np.float32(got) == acc


# ---- Gumbel quantiser: oracle/gumbel_oracle.py against the reference module's own outputs (tests/golden/gumbel_*.npz) ----------
import glob as _glob
import os as _os

GUMBEL_CASES = sorted(_os.path.basename(p)[:-4] for p in _glob.glob(_os.path.join(_os.path.dirname(__file__), "golden", "gumbel_*.npz")))


def _gumbel_case(name):
    return dict(np.load(_os.path.join(_os.path.dirname(__file__), "golden", name + ".npz")))


@pytest.mark.parametrize("name", GUMBEL_CASES)
def test_gumbel_oracle_matches_reference(name):
    from oracle import gumbel_oracle as GO
    c = _gumbel_case(name)
    hard = bool(c["straight_through"]) if bool(c["is_training"]) else True          # GumbelQuantizer.py:54
    out = GO.forward(c["z"], c["W"], c["b"], c["E"], c["noise"], float(c["tau"]), hard, float(c["kld_scale"]))
    assert np.array_equal(out["ind"], c["ind"])
    np.testing.assert_allclose(out["z_q"], c["z_q"], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(out["diff"], c["diff"], rtol=2e-5, atol=1e-9)
    g = GO.forward_backward_torch(c["z"], c["W"], c["b"], c["E"], c["noise"], float(c["tau"]), hard, float(c["kld_scale"]), c["G"], float(c["c"]))
    for k in ("grad_z", "grad_W", "grad_b", "grad_E"):
        np.testing.assert_allclose(g[k], c[k], rtol=1e-3, atol=5e-5, err_msg=k)      # conv1d vs matmul summation order


def test_gumbel_golden_set_is_complete():
    assert len(GUMBEL_CASES) == 5 and "gumbel_eval" in GUMBEL_CASES
