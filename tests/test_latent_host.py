"""Host side of the latent analyses (no GPU): the C ABI validates before it launches, LatentCensus and the tensor wrappers refuse
what they cannot serve, the f64 restatements of tests/_latent_ref.py say what plain torch says, and the filter of
analyses/get_max_acc_sentences.py keeps the rows the reference's file keeps."""
import os

import pytest
import torch

import _latent_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "kindergarten-vq-vae_amd")


def _lib():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(PKG, "lib", "libkvq.so")):
        g.build()
    from kvq import _ffi
    return _ffi.lib()


def test_group_sum_workspace_is_one_padded_f64_slab_per_run_and_group():
    """Runs of max(8, ceil(B / 256)) sentences (the rule beside the kernels in csrc/kvq_latent.hip); a slab's [S * H] plane is padded
    to an even number of cells."""
    lib = _lib()
    up = lambda n: (n + 255) // 256 * 256
    q = lib.kvq_latent_group_sum_workspace_bytes
    assert q(1, 12, 128, 3) == up(1 * 3 * 12 * 128 * 8)
    assert q(9, 12, 128, 3) == up(2 * 3 * 12 * 128 * 8)
    assert q(70, 12, 128, 3) == up(9 * 3 * 12 * 128 * 8)
    assert q(2048, 12, 768, 2) == up(256 * 2 * 12 * 768 * 8)            # runs of 8
    assert q(100000, 12, 768, 2) == up(256 * 2 * 12 * 768 * 8)          # runs of 391: never more than 256 slabs
    assert q(5, 3, 5, 1) == up(1 * 1 * 16 * 8)                          # 15 cells padded to 16
    assert q(0, 12, 128, 3) == 0


def test_the_three_entry_points_validate_before_any_launch():
    lib = _lib()
    fake = 4096

    def gsum(x=fake, ldx=128, B=4, S=12, H=128, G=3, io=1, table=fake, ws=fake, ws_bytes=1 << 30):
        return lib.kvq_latent_group_sum(x, ldx, fake, B, S, H, G, io, table, fake, None, ws, ws_bytes, None)

    def shift(x=fake, ldx=128, g1=1, g0=0, B=4, S=12, H=128, G=3, io=1, out=fake, ldo=128):
        return lib.kvq_latent_shift(x, ldx, fake, fake, g1, g0, 1.0, None, B, S, H, G, io, out, ldo, None)

    def lookup(idx=fake, N=4, K=32, Dg=128, G=1, io=1, out=fake, ldo=128):
        return lib.kvq_vq_lookup(idx, fake, N, K, Dg, G, io, out, ldo, None, None)
    for fn, kw, rc, text in ((gsum, dict(x=None), -1, b"null pointer"), (gsum, dict(H=0), -1, b"required"), (gsum, dict(io=5), -1, b"io_dtype"),
                             (gsum, dict(ldx=100), -1, b"row stride"), (gsum, dict(ws=None), -2, b"workspace"),
                             (gsum, dict(ws_bytes=64), -2, b"workspace"), (gsum, dict(table=4104), -1, b"16-byte"),
                             (shift, dict(out=None), -1, b"null pointer"), (shift, dict(g1=3), -1, b"outside"),
                             (shift, dict(g0=-1), -1, b"outside"), (shift, dict(ldo=64), -1, b"row strides"), (shift, dict(io=2), -1, b"io_dtype"),
                             (lookup, dict(idx=None), -1, b"null pointer"), (lookup, dict(K=0), -1, b"required"),
                             (lookup, dict(G=3, ldo=128), -1, b"row stride"), (lookup, dict(io=9), -1, b"io_dtype")):
        assert fn(**kw) == rc, (fn.__name__, kw)
        assert text in lib.kvq_last_error(), (fn.__name__, kw, lib.kvq_last_error())
    assert gsum(B=0) == 0 and shift(B=0) == 0 and lookup(N=0) == 0           # nothing to do: no launch either


def test_latent_census_and_the_wrappers_refuse_cpu_tensors_and_bad_sizes():
    from kvq import nnops
    from kvq._ffi import KvqError
    from kvq.census import LatentCensus
    with pytest.raises(KvqError, match="no CPU path"):
        LatentCensus(2, 12, 128, device="cpu")
    for bad in ((0, 12, 128), (2, 0, 128), (2, 12, 0)):
        with pytest.raises(KvqError, match=">= 1"):
            LatentCensus(*bad, device="cuda")
    x = torch.zeros(4, 12, 128)
    table, count = torch.zeros(3, 12, 128, dtype=torch.float64), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(KvqError, match="CPU tensor"):
        nnops.latent_group_sum(x, torch.zeros(4, dtype=torch.int32), table, count)
    with pytest.raises(KvqError, match="CPU tensor"):
        nnops.latent_shift(x, table, count, 1, 0)
    with pytest.raises(KvqError, match="CPU tensor"):
        nnops.vq_lookup(torch.zeros(4, 1, dtype=torch.int64), torch.zeros(32, 128), 32, torch.float32)
    census = LatentCensus.__new__(LatentCensus)                 # the checks of add() / shift() in front of the device work
    census.G, census.S, census.H, census.device = 2, 12, 128, torch.device("cuda", 0)
    with pytest.raises(KvqError, match="CPU tensor"):
        census.add(x, 0)
    with pytest.raises(KvqError, match="CPU tensor"):
        census.shift(x, 1, 0)


def test_group_sum_restatement_against_plain_torch():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(7, 3, 5, generator=g)
    group = torch.tensor([0, 2, -1, 0, 5, 2, -2])
    table, count, mag, n_bad = R.group_sum_ref(x, group, 3)
    assert count.tolist() == [2, 0, 2] and n_bad == 2
    torch.testing.assert_close(table[0], (x[0].double() + x[3].double()), rtol=0, atol=0)
    torch.testing.assert_close(table[2], (x[1].double() + x[5].double()), rtol=0, atol=0)
    assert float(table[1].abs().max()) == 0.0
    torch.testing.assert_close(mag[0], x[0].double().abs() + x[3].double().abs(), rtol=0, atol=0)
    want = R.mean_direction_ref(x, group, 2, 0)
    torch.testing.assert_close(table[2] / 2 - table[0] / 2, want, rtol=0, atol=1e-15)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_shift_restatement_against_plain_torch(dtype):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 3, 8, generator=g).to(dtype)
    table = torch.randn(2, 3, 8, generator=g, dtype=torch.float64) * 5
    count = torch.tensor([5, 3])
    sel = torch.tensor([[1, 0, 1]] * 4, dtype=torch.int8)
    got = R.shift_ref(x, table, count, 1, 0, alpha=0.5, sel=sel)
    assert got.dtype == dtype and torch.equal(got[:, 1], x[:, 1])                  # unselected positions: the same bits
    want = x.double() + 0.5 * (table[1] / 3 - table[0] / 5)
    # one rounding to f32 and one to the io dtype: half an ulp of each format (2^-24, 2^-8 relative) bounds the distance
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -24
    err = (got.double() - want)[:, [0, 2]].abs()
    assert bool((err <= 1.001 * eps * want[:, [0, 2]].abs() + 1e-30).all())
    assert torch.equal(R.shift_ref(x, table, count, 1, 0, alpha=0.0), x)
    assert torch.equal(R.shift_ref(x, table, torch.tensor([0, 3]), 1, 0), x)       # an empty group: no shift


def test_lookup_restatement_against_plain_torch():
    g = torch.Generator().manual_seed(2)
    K, Dg = 5, 4
    E = torch.randn(3 * K, Dg, generator=g)
    idx = torch.randint(0, K, (6, 3), generator=g)
    got = R.lookup_ref(E, idx, K, torch.bfloat16)
    assert got.shape == (6, 12) and got.dtype == torch.bfloat16
    for n in range(6):
        for f in range(3):
            assert torch.equal(got[n, f * Dg:(f + 1) * Dg], E[f * K + int(idx[n, f])].bfloat16())
    one = R.lookup_ref(E[:K], idx[:, :1], K, torch.float32)
    assert torch.equal(one, E[:K][idx[:, 0]])


def test_max_acc_filter_keeps_the_perfect_rows_sorted_by_input_sentence(tmp_path):
    import pandas as pd
    from analyses import get_max_acc_sentences as G
    df = pd.DataFrame({"epoch": [1] * 6, "stage": ["test"] * 6,
                       "input_sentence": ["they are touring the lakes", "he accepted the payment", "we did not open a door",
                                          "are you not ruining the holidays", "i count some coins", "she is loading the trucks"],
                       "recon_sentence": ["x"] * 6, "sentence_acc": [1.0, 0.9990, 0.99901, 0.5, 1.0, 0.0],
                       "verb_tense": ["present", "past", "past", "present", "present", "present"]})
    kept = G.max_acc_only(df)
    assert kept["input_sentence"].tolist() == ["i count some coins", "they are touring the lakes", "we did not open a door"]
    assert kept["index"].tolist() == [4, 0, 2]                  # reset_index() keeps the old row number as a column
    assert kept.index.tolist() == [0, 1, 2] and bool((kept["sentence_acc"] > 0.999).all())
    assert set(df.columns) <= set(kept.columns)
    assert len(G.max_acc_only(df, threshold=0.4)) == 5
    # the table round-trips through the file the entry points write, feather or the csv fallback
    path = G.write_table(df, str(tmp_path / "decoded_sentences.feather"))
    assert os.path.exists(path)
    back = G.read_table(str(tmp_path / "decoded_sentences.feather"))
    assert G.max_acc_only(back)["input_sentence"].tolist() == kept["input_sentence"].tolist()
    df.to_csv(tmp_path / "only_csv.csv", index=False)
    assert len(G.read_table(str(tmp_path / "only_csv.feather"))) == 6
    with pytest.raises(FileNotFoundError):
        G.read_table(str(tmp_path / "absent.feather"))
