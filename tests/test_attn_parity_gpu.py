"""The bf16 attention kernels of the step (csrc/kvq_nn.hip: attn_fwd_mfma_kernel, attn_bwd_mfma_kernel, and the blocked
33 .. 128-token kernels attn_fwd_blk_kernel, attn_bwd_blk_dq_kernel, attn_bwd_blk_dkv_kernel) against the f64 reference of
tests/_attn_ref.py, judged per (sentence, head, row) with the dropout mask the kernel really drew, in the layouts, strides and
batch sizes of the engine, every output inside a frame that must stay untouched bit for bit (tests/_attn_case.py).

Every case prints `ATTN-RATIO <family> <case> {output: worst |got - ref| / env}` before it asserts; the margins in
tests/_attn_ref.py::MARGIN are set from one such run."""
import os
import subprocess
import sys

import pytest
import torch

import _attn_case as C
import _attn_ref as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from kvq import _ffi
    _ffi.lib()
    assert torch.cuda.is_available()
    assert _ffi.lib().kvq_attn_set_variant(2) == 0


def _report(label, ratios):
    print("ATTN-RATIO", label, {k: round(v, 3) for k, v in ratios.items()})


def check(label, **kw):
    """run the kernels (frames asserted inside), reveal the mask they drew, judge every output against the f64 reference"""
    inputs, got = C.run(**kw)
    B, nh, Sq, Sk, p = kw["B"], kw["nh"], kw["Sq"], kw["Sk"], kw["p"]
    keep = C.reveal_keep(B, nh, Sq, Sk, p, kw.get("seed", 1), kw.get("site", 3)) if p > 0 else None
    if keep is not None:
        rate = 1 - keep.mean().item()
        assert abs(rate - p) < 0.03 + 2.0 / (B * nh * Sq * Sk) ** 0.5, rate
    family = "mfma" if Sq <= 32 and Sk <= 32 else "blk"
    args = (inputs["q"], inputs["k"], inputs["v"], inputs["mask"], kw["causal"], 0.125, keep, p, inputs["g_out"])
    ref = A.reference(*args)
    mod = A.model(*args, family=family)
    for name, t in got.items():
        assert torch.isfinite(t).all(), f"{label}: {name} has a non-finite value"
    floors = A.cancellation_floors(inputs["q"], inputs["k"], inputs["v"], inputs["g_out"], inputs["mask"], kw["causal"], 0.125) if family == "blk" else None
    A.judge_all(got, ref, mod, A.MARGIN[family], f"{family} {label}", _report, floors)
    return inputs, got, ref, mod


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("causal", [False, True])
def test_step_shape(causal, p):
    """B = 256, nh = 12, S = 32: 3072 workgroups; q / k / v the column thirds of one [8192, 2304] buffer, the gradients the thirds of
    another; key-padding lengths in [1, 32]; bias partials requested."""
    check(f"step causal={causal} p={p}", B=256, nh=12, Sq=32, Sk=32, causal=causal, mask_kind="prefix", p=p, layout="qkv", cpad=0)


def test_step_shape_in_a_column_frame():
    check("step framed", B=256, nh=12, Sq=32, Sk=32, causal=True, mask_kind="prefix", p=0.1, layout="qkv", cpad=8)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("Sq,Sk", [(9, 12), (12, 9), (32, 12), (7, 32), (32, 5), (1, 32), (32, 1)])
def test_cross_attention_in_the_engine_layout(Sq, Sk, p):
    """k / v = layer 5's column slices of a [B*Sk, 12 * 2H] buffer (row stride 18432), gradients and k / v bias partials into the
    same slices; no encoder mask, as in the step."""
    check(f"cross {Sq}x{Sk} p={p}", B=8, nh=12, Sq=Sq, Sk=Sk, causal=False, mask_kind=None, p=p, layout="cross")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S", [1, 2, 5, 31])
def test_ragged_and_small(S, causal):
    """one sentence, one head; then a batch under a mask with holes (some sentences without key 0, so that causal leaves their first
    queries without any key) whose last sentence is the shortest -- the whole-line stores of a short sentence must leave the rows
    of the next one, the columns beside the head range and the memory after the last sentence alone (frames, asserted in run())."""
    check(f"single S={S} causal={causal}", B=1, nh=1, Sq=S, Sk=S, causal=causal, mask_kind=None, p=0.1, layout="qkv")
    check(f"holes S={S} causal={causal}", B=5, nh=3, Sq=S, Sk=S, causal=causal, mask_kind="holes" if S > 1 else None, p=0.1,
          layout="qkv")
    check(f"holes cross S={S}", B=5, nh=3, Sq=S, Sk=max(1, S - 1), causal=False, mask_kind="holes" if S > 2 else None, p=0.0,
          layout="cross", L=3, layer=1)


BLK = [(33, 33), (64, 64), (65, 65), (96, 96), (127, 127), (128, 128), (40, 96), (20, 70), (70, 20)]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("Sq,Sk", BLK)
def test_blocked_kernels(Sq, Sk, p):
    """33 .. 128 tokens, B = 64, nh = 12, through ctx= / lse= of nnops.attn_bwd: causal (self-attention sizes) and key-padded; the
    sizes with a ragged and with a full last block also key-padded without causal."""
    if Sq == Sk:
        check(f"blk {Sq}x{Sk} causal p={p}", B=64, nh=12, Sq=Sq, Sk=Sk, causal=True, mask_kind="prefix", p=p, layout="qkv")
        if Sq in (65, 128):
            check(f"blk {Sq}x{Sk} masked p={p}", B=64, nh=12, Sq=Sq, Sk=Sk, causal=False, mask_kind="prefix", p=p, layout="qkv")
    else:
        check(f"blk {Sq}x{Sk} masked p={p}", B=64, nh=12, Sq=Sq, Sk=Sk, causal=False, mask_kind="prefix", p=p, layout="cross", L=2,
              layer=1)


@pytest.mark.parametrize("S,causal", [(32, False), (12, True), (64, False), (100, True)])
def test_sentence_without_any_attended_key(S, causal):
    """A mask row of zeros next to normal sentences.  The contract (include/kvq.h, kvq_attn_fwd): that sentence's context rows, its
    gradient rows and its bias partial rows are exactly 0 and its lse is log(1e-37) -- no NaN, where HuggingFace's additive mask
    gives uniform attention over the padding.  Everything else passes the judge as if the sentence were not there."""
    inputs, got, ref, mod = check(f"empty S={S} causal={causal}", B=5, nh=3, Sq=S, Sk=S, causal=causal, mask_kind="empty2", p=0.1,
                                  layout="qkv")
    for name in A.OUTPUTS:
        assert not got[name][2].any(), name
    torch.testing.assert_close(got["lse"][2], torch.full_like(got["lse"][2], A.LSE_EMPTY), rtol=2.0 ** -18, atol=0)


def test_requesting_partials_changes_no_other_output():
    """... bit for bit; and without them the partial buffers keep their pattern entirely (asserted in run())."""
    inputs, got = C.run(B=3, nh=2, Sq=32, Sk=32, causal=False, mask_kind="prefix", p=0.0, layout="qkv", partials=False)
    _, got2 = C.run(B=3, nh=2, Sq=32, Sk=32, causal=False, mask_kind="prefix", p=0.0, layout="qkv", partials=True)
    for name in ("ctx", "lse", "g_q", "g_k", "g_v"):          # asking for the partials changes no other output
        assert torch.equal(got[name], got2[name]), name


ARMS = [("default", {"KVQ_ATTN_COAL": "1", "KVQ_ATTN_STC": "1"}), ("rows per lane", {"KVQ_ATTN_COAL": "0"}),
        ("16-byte stores", {"KVQ_ATTN_COAL": "1", "KVQ_ATTN_STC": "0"})]


def test_the_load_and_store_arms_are_bit_identical(tmp_path):
    """KVQ_ATTN_COAL=0 and KVQ_ATTN_STC=0 change how rows are loaded and stored, not the arithmetic: one fresh child process per arm,
    one at a time, each computing tests/_attn_case.py::ARM_CASES; the outputs must equal the default arm's bit for bit."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_attn_case.py")
    results = {}
    for name, env in ARMS:
        out = tmp_path / (name.replace(" ", "_") + ".pt")
        r = subprocess.run([sys.executable, child, str(out)], env={**os.environ, **env}, timeout=300, capture_output=True, text=True)
        assert r.returncode == 0, f"arm '{name}' ended with status {r.returncode}; nothing more is started:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
        results[name] = torch.load(out)
    base = results["default"]
    for name, _ in ARMS[1:]:
        for case, outs in base.items():
            for key, t in outs.items():
                o = results[name][case][key]
                same = torch.equal(t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32),
                                   o.view(torch.int16) if o.dtype == torch.bfloat16 else o.view(torch.int32))
                assert same, f"arm '{name}', case {case}: {key} differs from the default arm in {(t != o).sum().item()} elements"
